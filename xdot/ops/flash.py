"""Python face of the flash-attention kernels (``csrc/flash_fwd.hip``, ``csrc/flash_bwd.hip``,
``csrc/mask_pack.hip``).

Tensors are head-interleaved: ``rows`` (B, R, H*D) local query-side rows, ``kc``/``vc``
(B, T, Hg*D) the gathered key/value side.  ``Hg`` (None: ``H``) is the number of gathered heads:
with ``Hg < H`` (grouped-query attention) row head ``h`` reads gathered head ``h // (H // Hg)`` and
the gathered-side gradients are summed over each group in the column kernel (16-bit, D <= 128).  The RCCL all-gather produces rank-major
(N, B, Rc, H*D); :func:`gathered_to_btc` turns that into (B, T, H*D) (a free view for B = 1)
and :func:`btc_to_rank_major` maps the fp32 key/value-side gradients back for the
reduce-scatter.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _ext
from ..utils.env import FLAGS
from .mask import GatheredColumns, StructuredMask, segments_of


class PackedMask:
    """Boolean (B, R, T) mask compressed to per-row bit words ``bits`` (B, ceil(T/64), R),
    the same bits column-major per 64-row tile ``bits_t`` (B, ceil(R/64), Tpad) for the
    backward column kernel, and per (32-row, 64-col) tile ``flags`` (0 none / 1 all / 2 some
    masked)."""

    __slots__ = ("bits", "flags", "bits_t", "shape")

    def __init__(self, bits: torch.Tensor, flags: torch.Tensor, bits_t: torch.Tensor, shape):
        self.bits, self.flags, self.bits_t, self.shape = bits, flags, bits_t, tuple(shape)

    @property
    def nothing_masked(self) -> bool:  # host sync; diagnostics only
        return bool((self.flags == 0).all())


def prepare_mask(mask: Optional[torch.Tensor], B: int, R: int, T: int) -> Optional[PackedMask]:
    if mask is None:
        return None
    if tuple(mask.shape) != (B, R, T):
        raise ValueError(f"mask must be (B, R, T) = {(B, R, T)}, got {tuple(mask.shape)}")
    bits, flags, bits_t = _ext.ops().mask_pack(mask.to(torch.bool).contiguous())
    return PackedMask(bits, flags, bits_t, mask.shape)


def generate_mask(spec: StructuredMask, B: int, R: int, T: int, row_offset: Optional[int] = None, segments=None,
                  device=None, row_segments=None) -> PackedMask:
    """The packed form of ``spec`` for ``R`` local rows starting at global row ``row_offset`` and
    ``T`` packed columns, generated on the GPU (``mask_gen`` in ``csrc/mask_pack.hip``): bitwise
    what :func:`prepare_mask` gives for ``spec.dense(...)``, with nothing R x T sized allocated.

    ``segments``: the packed columns as runs ``(packed_start, length, global_start)`` of
    consecutive global columns (``global_start = -1``: a run that is always masked); None: the
    identity, packed column = global column.  ``row_offset`` is used where ``spec`` has none;
    ``device``: default the device of ``spec.lengths`` (else of ``spec.doc_starts``) when on a
    GPU, else the current one.

    ``row_segments``: the local rows as runs ``(local_start, length, global_start)`` of consecutive
    global rows (:func:`xdot.parallel.layout.row_runs`) in place of ``row_offset``; they must tile
    the ``R`` rows exactly.  One run starting at local row 0 is the ``row_offset`` call."""
    spec.check(B)
    rows = None
    if row_segments is not None:
        rows = [tuple(int(x) for x in rn) for rn in row_segments]
        if R > 0 and sorted((a, a + n) for a, n, _g in rows if n > 0) != _tiling(rows, R):
            raise ValueError(f"generate_mask: the row segments must tile the {R} rows exactly, got {rows}")
        if any(g < 0 or g + n > 2**31 - 1 for _a, n, g in rows):
            raise ValueError(f"generate_mask: the row segments' global rows must lie in [0, 2^31), got {rows}")
        if spec.row_offset is not None:
            raise ValueError("generate_mask: row_segments contradict the mask's explicit row_offset")
        rows = [rn for rn in rows if rn[1] > 0]
        if len(rows) <= 1:  # consecutive rows: the row_offset launch
            row_offset, rows = (rows[0][2] if rows else 0), None
    ro = 0 if rows is not None else (spec.row_offset if spec.row_offset is not None else row_offset)
    if ro is None:
        raise ValueError("generate_mask: row_offset is not set")
    if device is None:
        on_gpu = [t for t in (spec.lengths, spec.doc_starts) if t is not None and t.is_cuda]
        device = on_gpu[0].device if on_gpu else torch.device("cuda", torch.cuda.current_device())
    segs = [(0, T, 0)] if segments is None else [tuple(int(x) for x in sg) for sg in segments]
    if sorted((p, p + n) for p, n, _g in segs if n > 0) != _tiling(segs, T):
        raise ValueError(f"generate_mask: the segments must tile the {T} packed columns exactly, got {segs}")
    table = torch.tensor(segs or [(0, 0, 0)], dtype=torch.int32).reshape(-1, 3).to(device, non_blocking=True)
    ds = spec.device_doc_starts(device)
    # (trailing arguments only when set: an extension built before they existed takes every other call)
    tail = (() if ds is None else (ds,)) if rows is None else (
        ds, torch.tensor(rows, dtype=torch.int32).reshape(-1, 3).to(device, non_blocking=True))
    bits, flags, bits_t = _ext.ops().mask_gen(int(B), int(R), int(T), spec.causal, int(spec.window or 0), int(ro),
                                              spec.device_lengths(device), table, *tail)
    return PackedMask(bits, flags, bits_t, (B, R, T))


def _tiling(segs, T: int):
    """[(start, end)] of the non-empty segments if they cover [0, T) back to back, else None."""
    out, at = [], 0
    for p, e in sorted((p, p + n) for p, n, _g in segs if n > 0):
        if p != at:
            return None
        out.append((p, e))
        at = e
    return out if at == T else None


class _MaskEntry:
    __slots__ = ("ref", "version", "packed", "none_ev", "none_host")


class MaskCache:
    """Packed masks keyed on the boolean tensor (or :class:`StructuredMask`) that produced them.

    A training loop passes the same mask object every step (the reference's ``example.py``
    builds it once); re-packing it costs a full read of the (B, R, T) bool tensor per step
    (625 MB at T = 25000, N = 1).  An entry is valid while the tensor is alive (a weak
    reference whose finaliser evicts the entry, so a new tensor at a recycled address never
    hits) and its ``_version`` — bumped by every in-place write — is unchanged.

    All-False short-circuit: when a mask is packed, "any tile masked?" is copied to pinned host
    memory without a sync; on a later hit whose copy has landed and reads False, the cache
    hands out ``None`` (the kernels' no-mask path, nothing to stage per tile)."""

    def __init__(self, capacity: int = 8):
        self.capacity = capacity
        self._d = {}

    def _evict(self, key):
        self._d.pop(key, None)

    def get(self, mask: torch.Tensor, tag, pack):
        """``pack()`` -> PackedMask on a miss; ``tag`` distinguishes views packed from the
        same tensor (row chunks)."""
        import weakref

        key = (id(mask), tag)
        e = self._d.get(key)
        if e is not None and e.ref() is mask and e.version == mask._version:
            if e.none_ev is not None and e.none_ev.query():
                if not bool(e.none_host.item()):
                    return None
                e.none_ev = None
            return e.packed
        packed = pack()
        if packed is None:
            return None
        e = _MaskEntry()
        e.ref = weakref.ref(mask, lambda _r, k=key, c=self: c._evict(k))
        e.version = mask._version
        e.packed = packed
        e.none_ev, e.none_host = None, None
        if packed.flags.is_cuda:
            e.none_host = torch.empty((), dtype=torch.bool, pin_memory=True)
            # the flag rows are padded to a multiple of 4 tiles with 1 ("all masked"): only the
            # ceil(T/64) real column tiles count
            nkt = (packed.shape[-1] + 63) // 64
            e.none_host.copy_(packed.flags[..., :nkt].any(), non_blocking=True)
            e.none_ev = torch.cuda.Event()
            e.none_ev.record()
        if len(self._d) >= self.capacity:
            self._d.pop(next(iter(self._d)))
        self._d[key] = e
        return packed

    def clear(self):
        self._d.clear()


MASK_CACHE = MaskCache()


def prepare_mask_cached(mask: Optional[torch.Tensor], B: int, R: int, T: int, tag=None,
                        view=None) -> Optional[PackedMask]:
    """:func:`prepare_mask` through :data:`MASK_CACHE` (``view(mask)``: the slice to pack).

    ``mask`` may be a bound :class:`StructuredMask` (``StructuredMask.bind``: row offset resolved,
    global column count known): the packed mask is then generated, ``view`` giving the column
    segment table (:func:`xdot.ops.mask.segments_of`) instead of a sliced tensor."""
    if mask is None:
        return None
    if isinstance(mask, StructuredMask):
        if mask._T is None:
            raise ValueError("prepare_mask_cached: bind() the StructuredMask first (row offset, global columns)")
        # (one description serves any batch / row count, unlike a tensor: the shape is part of the key)
        return MASK_CACHE.get(mask, (tag, B, R, T),
                              lambda: generate_mask(mask, B, R, T, segments=segments_of(view, mask._T, mask._cols),
                                                    row_segments=mask._rows))
    if isinstance(mask, GatheredColumns):
        # a dense tensor with global columns under a layout: its columns go into gathered order
        # first (one R x T byte copy per miss, as a chunk permutation makes), then the launch's view
        sel = mask.select if view is None else (lambda m: view(mask.select(m)))
        return MASK_CACHE.get(mask.tensor, ("cols", mask.key, tag), lambda: prepare_mask(sel(mask.tensor), B, R, T))
    return MASK_CACHE.get(mask, tag, lambda: prepare_mask(mask if view is None else view(mask), B, R, T))


class PendingMask:
    """A mask being packed on a side stream (:func:`prepare_mask_async`): the packing overlaps
    whatever the current stream does meanwhile (the projection GEMMs); :meth:`get` orders the
    calling stream after it."""

    __slots__ = ("raw", "shape", "_packed", "_event")

    def __init__(self, raw: torch.Tensor, packed: PackedMask, event):
        self.raw, self.shape, self._packed, self._event = raw, tuple(raw.shape), packed, event

    def get(self) -> Optional[PackedMask]:
        cur = torch.cuda.current_stream(self.raw.device)
        cur.wait_event(self._event)
        if self._packed is None:  # cached all-False mask
            return None
        for t in (self._packed.bits, self._packed.flags, self._packed.bits_t):
            t.record_stream(cur)
        return self._packed


_AUX = {}


def prepare_mask_async(mask: torch.Tensor, B: int, R: int, T: int) -> PendingMask:
    """:func:`prepare_mask` on a per-device side stream, ordered after the current stream."""
    dev = mask.device
    i = dev.index if dev.index is not None else torch.cuda.current_device()
    if i not in _AUX:
        _AUX[i] = torch.cuda.Stream(device=i)
    side = _AUX[i]
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        packed = prepare_mask_cached(mask, B, R, T)
        ev = torch.cuda.Event()
        ev.record(side)
    mask.record_stream(side)
    return PendingMask(mask, packed, ev)


def gathered_to_btc(g: torch.Tensor) -> torch.Tensor:
    """(N, B, Rc, C) rank-major all-gather output -> (B, N*Rc, C)."""
    N, B, Rc, C = g.shape
    if B == 1:
        return g.view(1, N * Rc, C)
    return g.permute(1, 0, 2, 3).reshape(B, N * Rc, C)


def btc_to_rank_major(x: torch.Tensor, N: int) -> torch.Tensor:
    """(B, T, C) -> (N, B, T/N, C) contiguous (reduce-scatter send layout)."""
    B, T, C = x.shape
    if B == 1:
        return x.view(N, 1, T // N, C)
    return x.view(B, N, T // N, C).permute(1, 0, 2, 3).contiguous()


def _kv(x: torch.Tensor) -> torch.Tensor:
    """key/value-side operand: (B, T, C) with unit inner stride (row stride may exceed C)."""
    if x.dim() == 3 and x.stride(-1) == 1 and x.stride(1) % 8 == 0 and (x.shape[0] == 1 or x.stride(0) == x.shape[1] * x.stride(1)):
        return x
    return x.contiguous()


def _hg(Hg: Optional[int]):
    """The ops' trailing ``Hg`` argument: passed only when set (an extension built before it existed
    -- an A/B build loaded through ``XDOT_EXT_PATH`` -- still takes every other call)."""
    return (int(Hg),) if Hg else ()


def _mask_args(mk: Optional[PackedMask]):
    return (mk.bits, mk.flags) if mk is not None else (None, None)


def prescale(rows: torch.Tensor, scale: float) -> torch.Tensor:
    """``rows * (scale * log2 e)`` in the input dtype (one rounding), the form the kernels take with
    ``prescaled=True``: their score accumulators are then seeded with the row max / LSE and the
    probabilities are ``2^acc`` with no per-score FMA.  Forward and backward must see the SAME
    pre-scaled buffer."""
    return _ext.ops().flash_prescale(rows.contiguous(), float(scale))


FP32_MODES = {"exact": 0, "split": 1, "split3": 2}


def fp32_code(dtype: torch.dtype, mode: Optional[str] = None) -> int:
    """Kernel family of fp32 operands: 0 exact fp32 (``csrc/flash_f32.hip``, the default: ~5e-7
    relative error vs fp64, the reference's precision), 1 split-bf16 (``csrc/flash_x3.hip``,
    opt-in: 3 bf16 MFMAs per product, <= 9e-6; profiles/r3_fp32_split.md), 2 split3
    (``csrc/flash_x6.hip``, opt-in: three bf16 parts per operand, 6 bf16 MFMAs per product, the exact
    family's error; D <= 128, no S buffer: a dS buffer or recompute; profiles/split3.md).
    ``mode`` None: ``XDOT_FP32_MODE``.  0 for 16-bit dtypes."""
    if dtype != torch.float32:
        return 0
    mode = FLAGS.fp32_mode if mode is None else mode
    if mode not in FP32_MODES:
        raise ValueError(f"fp32 mode must be one of {sorted(FP32_MODES)}, got {mode!r}")
    return FP32_MODES[mode]


def score_buffer_numel(B: int, H: int, R: int, T: int) -> int:
    """Floats of the fp32 score buffer: (B*H, ceil(R/32), ceil(T/32)) blocks of 32x32, plus one
    dump block the waves that own no block (rows past R, columns past T) write into."""
    return (B * H * ((R + 31) // 32) * ((T + 31) // 32) + 1) * 1024


def _score_room(device) -> float:
    """Bytes the score buffers may take: ``XDOT_FP32_SCORES_FRAC`` of the memory free on the
    device (free + cached by torch)."""
    free, _ = torch.cuda.mem_get_info(device)
    cached = torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
    return FLAGS.fp32_scores_frac * (free + cached)


def score_buffer(B: int, H: int, R: int, T: int, device) -> Optional[torch.Tensor]:
    """The fp32 score buffer (``csrc/flash_f32.hip`` exact, ``csrc/flash_x3.hip`` split; score-buffer mode) or None.

    The forward stores every computed score tile there; the backward's column kernel reads S
    instead of recomputing it and overwrites it with dS, which the row kernel reads: 6 fp32
    products per step instead of 9 for 8 bytes of otherwise idle HBM traffic per score.  It is
    R x T x H floats (20 GB at T = R = 25000, H = 8), so it is only taken when it fits within
    ``XDOT_FP32_SCORES_FRAC`` of the memory free on the device (free + cached by torch); else
    None and the kernels recompute (``XDOT_FP32_SCORES=0`` forces that)."""
    if not FLAGS.fp32_scores:
        return None
    n = score_buffer_numel(B, H, R, T)
    dev = torch.device(device)
    if 4 * n > _score_room(dev):
        return None
    return torch.empty(n, dtype=torch.float32, device=dev)


def fused_cols_wanted(fp32_mode: int, D: int) -> bool:
    """The exact-fp32 backward's column side as ONE fused pass (dP, dQ and dV per tile, S
    overwritten with dS in place; ``XDOT_F32_FUSED_COLS``) instead of a dQ pass and a dV pass:
    exact family, D <= 128."""
    return FLAGS.f32_fused_cols and fp32_mode == 0 and D <= 128


def score_buffers(B: int, H: int, R: int, T: int, device, dsbuf: bool = True):
    """(S buffer, dS buffer) for the backward's concurrent schedule, (S buffer, None) for the
    in-place one, or None (recompute): like :func:`score_buffer`, the dS buffer only when both fit
    within ``XDOT_FP32_SCORES_FRAC`` of the free device memory.  With a separate dS buffer the
    column side runs its dQ pass first (S -> dS), then its dV pass (reads S) CONCURRENTLY with the
    row kernel (reads dS): two one-product kernels side by side instead of back to back.
    ``dsbuf=False``: the S buffer only (in place)."""
    if not FLAGS.fp32_scores:
        return None
    n = score_buffer_numel(B, H, R, T)
    dev = torch.device(device)
    room = _score_room(dev)
    if 8 * n <= room and FLAGS.fp32_scores_dsbuf and dsbuf:
        both = torch.empty(2 * n, dtype=torch.float32, device=dev)
        return both[:n], both[n:]
    if 4 * n <= room:
        return torch.empty(n, dtype=torch.float32, device=dev), None
    return None


def ds_only_wanted(fp32_mode: int, D: int) -> bool:
    """Whether fp32 family ``fp32_mode`` (0 exact, 1 split, 2 split3) at head dim ``D`` keeps only a dS
    buffer (``XDOT_FP32_DS_ONLY``): the forward stores nothing, the single-pass column kernel
    recomputes S and stores dS, the row kernel reads dS.  The split family's kernels are bound by
    the score traffic (S written, read twice, dS written and read: 100 GB per step at T = R =
    25000, H = 8); this mode moves 40 GB for one recomputed product on the column side.  split3 has
    no S-buffer kernels: it keeps the dS buffer unless ``XDOT_FP32_DS_ONLY=none`` (then it recomputes)."""
    if D > 128:
        return False
    m = FLAGS.fp32_ds_only
    return m == "all" or (m == "split" and fp32_mode == 1) or (m != "none" and fp32_mode == 2)


def fwd(rows: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, mk: Optional[PackedMask], H: int,
        scale: float, nsplit: int = 0, prescaled: bool = False,
        fp32_mode: Optional[int] = None, sbuf: Optional[torch.Tensor] = None,
        Hg: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (out (B, R, H*D) in rows.dtype, lse (B, H, R) fp32 natural log).

    ``nsplit``: column splits (0 = auto: split only when R is too small to fill the GPU).
    ``prescaled``: ``rows`` is :func:`prescale` output.  ``fp32_mode``: :func:`fp32_code`
    (None: from ``XDOT_FP32_MODE``).  ``sbuf``: fp32 (exact or split, not split3) only, a :func:`score_buffer` the
    raw scores are stored into for :func:`bwd_cols` / :func:`bwd_rows`."""
    bits, flags = _mask_args(mk)
    fm = fp32_code(rows.dtype) if fp32_mode is None else int(fp32_mode)
    return _ext.ops().flash_fwd(rows.contiguous(), _kv(kc), _kv(vc), bits, flags, int(H), float(scale), int(nsplit),
                                bool(prescaled), fm, sbuf, *_hg(Hg))


# ---- decode: a few new rows against one rank's cache (csrc/flash_decode.hip) ----------------------
DECODE_MAX_ROWS = 64   # G * Rn rows of one gathered head: four 16-row MFMA tiles
_FWD_HEAD_DIMS = (32, 64, 96, 128, 160, 192, 256, 384)


def decode_eligible(dtype: torch.dtype, D: int, Dv: int, G: int, Rn: int, cache_dtype=None) -> bool:
    """The decode kernel takes this call: 16-bit, one head dim of 32 / 64 / 96 / 128 for q and v, and at
    most 64 rows (``G`` row heads x ``Rn`` new rows) per gathered head.  More rows go to the row-blocked
    kernel (:func:`extend_eligible`), everything else to the forward kernels over a dense mask (:func:`decode`).  Every eligible shape that was measured is
    faster than that route (profiles/decode.md), so none is routed away.  ``dtype`` is the rows';
    ``cache_dtype`` ``torch.float8_e4m3fn`` asks for the fp8-cache kernel (csrc/flash_decode8.hip), which
    takes the same shapes; more rows over such a cache go to :func:`extend_fp8_eligible`."""
    if cache_dtype not in (None, dtype, torch.float8_e4m3fn):
        return False
    return (dtype in (torch.bfloat16, torch.float16) and D == Dv and D in (32, 64, 96, 128)
            and 1 <= G * Rn <= DECODE_MAX_ROWS)


def _pad_heads(x: torch.Tensor, h: int, Dp: int) -> torch.Tensor:
    """(B, L, h*d) -> (B, L, h*Dp): every head zero-padded to ``Dp`` features (``x`` itself for d = Dp)."""
    B, L, C = x.shape
    if C // h == Dp:
        return x
    return torch.nn.functional.pad(x.reshape(B, L, h, C // h), (0, Dp - C // h)).reshape(B, L, h * Dp)


def decode(rows: torch.Tensor, qc: torch.Tensor, vc: torch.Tensor, col_pos: torch.Tensor, pos0: int, H: int,
           scale: float, window: int = 0, Hg: Optional[int] = None, nsplit: int = 0,
           out_fp32: bool = False, qscale: Optional[torch.Tensor] = None,
           vscale: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Attention of ``Rn`` new rows over one rank's cache, forward only -> (out (B, Rn, H*Dv) in
    ``rows.dtype``, lse (B, H, Rn) fp32 natural log).

    ``rows`` (B, Rn, H*D): the new rows' ``k``, consecutive positions ``pos0, pos0 + 1, ...``, not
    pre-scaled.  ``qc`` / ``vc`` (B, Tcap, Hg*D): the cache, unit inner stride, any common row stride
    (the two halves of one ``[q|v]`` buffer).  ``col_pos`` (B, Tcap) int32: the global position of
    each slot, -1 = empty.  Slot ``c`` is visible to row ``i`` iff ``0 <= col_pos[b, c] <= pos0 + i``
    and (``window == 0`` or ``col_pos[b, c] > pos0 + i - window``): ``StructuredMask(causal=True,
    window=window)`` for those rows, evaluated in the kernel, so the cache may be filled in any order
    (contiguous, zigzag, round-robin appends) and no mask is built or packed.  Empty and invisible
    slots must still hold finite values (their probability 0 multiplies them).  A row that sees
    nothing comes out NaN with lse -inf, as from :func:`fwd`.

    ``nsplit``: column spans (0: ``plan_decode`` of ``csrc/flash_plan.h``).  ``out_fp32``: ``out`` in
    fp32, rounded once less (the wire format of :func:`xdot.decode_attention`'s cross-rank merge).

    16-bit calls with more than 64 rows per gathered head (chunked prefill, a long user turn, a long
    draft: :func:`extend_eligible`) run the row-blocked sweep of :func:`extend` under the same contract.
    Calls neither kernel takes (fp32, D > 128, Dv != D, more than 128 row heads per gathered head)
    run :func:`fwd` over the dense mask of the same rule, packed per call, with grouped heads
    repeated where :func:`fwd` has no grouped kernel and heads zero-padded to a common kernel width;
    CPU tensors and ``backend='torch'`` run ``xdot.parallel._ref.decode``.

    ``qscale`` / ``vscale`` (B, Hg, Tcap) fp32, unit inner stride: ``qc`` / ``vc`` are ``float8_e4m3fn`` and
    slot ``c`` of gathered head ``h`` stands for ``qscale[b, h, c] * qc[b, c, h*D:(h+1)*D]`` (and likewise
    ``v``): the format of :class:`xdot.AttnCache` with ``cache_dtype="fp8"``.  Eligible calls run the fp8
    sweep (csrc/flash_decode8.hip), which applies the scales per column and reads the bytes as they are, and
    with more than 64 rows per gathered head (:func:`extend_fp8_eligible`) its row-blocked form
    (csrc/flash_extend8.hip, :func:`extend`).  Only calls neither kernel takes (fp32 rows, D > 128, Dv != D,
    more than 128 row heads per gathered head) are the slow path: it first dequantises the whole cache into
    fp32 and runs the fp32 route of the call (the forward kernels over a dense mask on the GPU)."""
    B, Rn, C = rows.shape
    hg = int(Hg) if Hg else int(H)
    D, Dv, window = C // H, vc.shape[-1] // hg, int(window or 0)
    if qscale is not None:
        if vscale is None or qc.dtype != torch.float8_e4m3fn or vc.dtype != torch.float8_e4m3fn:
            raise ValueError("flash.decode: qscale and vscale go together, with float8_e4m3fn qc and vc")
        if _ext.use_hip(rows, qc, vc) and decode_eligible(rows.dtype, D, Dv, H // hg, Rn, torch.float8_e4m3fn):
            return _ext.ops().flash_decode_fp8(rows.contiguous(), _kv(qc), _kv(vc), qscale, vscale, col_pos, int(pos0),
                                               window, int(H), float(scale), hg, int(nsplit), bool(out_fp32))
        if _ext.use_hip(rows, qc, vc) and extend_fp8_eligible(rows.dtype, D, Dv, H // hg, Rn):
            return extend(rows, qc, vc, col_pos, pos0, H, scale, window, Hg, nsplit, out_fp32, qscale, vscale)
        from ..parallel import _ref

        # scale * byte does not fit a 16-bit value: a cache dequantised into rows.dtype would be rounded a
        # second time (measured: 2e-2 in the LSE at |scores| ~ 20), so the slow path computes in fp32
        cdt = _ref.compute_dtype(rows)
        qc, vc = ((t.to(cdt).reshape(B, -1, hg, t.shape[-1] // hg) * sc.to(cdt).transpose(1, 2).unsqueeze(-1)).reshape(t.shape)
                  for t, sc in ((qc, qscale), (vc, vscale)))
        if _ext.use_hip(rows, qc, vc):
            o, lse = decode(rows.to(cdt), qc, vc, col_pos, pos0, H, scale, window, Hg, nsplit, out_fp32=True)
            return (o if out_fp32 else o.to(rows.dtype)), lse
    if not _ext.use_hip(rows, qc, vc):
        from ..parallel import _ref  # (xdot.parallel imports this module)

        o, lse = _ref.decode(rows, qc, vc, col_pos, int(pos0), int(H), float(scale), window, Hg)
        return (o if out_fp32 else o.to(rows.dtype)), lse
    if decode_eligible(rows.dtype, D, Dv, H // hg, Rn):
        return _ext.ops().flash_decode(rows.contiguous(), _kv(qc), _kv(vc), col_pos, int(pos0), window, int(H),
                                       float(scale), hg, int(nsplit), bool(out_fp32))
    if extend_eligible(rows.dtype, D, Dv, H // hg, Rn, qc.dtype):
        return extend(rows, qc, vc, col_pos, pos0, H, scale, window, Hg, nsplit, out_fp32)
    from ..parallel._ref import decode_mask

    Dp = next((d for d in _FWD_HEAD_DIMS if d >= max(D, Dv)), None)
    if Dp is None:
        raise ValueError(f"flash.decode: head dims ({D}, {Dv}) above the forward kernels' {_FWD_HEAD_DIMS[-1]}")
    mk = prepare_mask(decode_mask(col_pos, int(pos0), Rn, window), B, Rn, qc.shape[1])
    rows_p, qc, vc = _pad_heads(rows, H, Dp), _pad_heads(qc, hg, Dp), _pad_heads(vc, hg, Dp)
    if hg != H and (rows.dtype == torch.float32 or Dp > 128):  # no grouped kernel there: heads repeated
        qc, vc = (t.reshape(B, -1, hg, Dp).repeat_interleave(H // hg, dim=2).reshape(B, -1, H * Dp) for t in (qc, vc))
        hg = H
    o, lse = fwd(rows_p, qc, vc, mk, H, scale, Hg=hg if hg != H else None)
    if Dp != Dv:
        o = o.reshape(B, Rn, H, Dp)[..., :Dv].reshape(B, Rn, H * Dv)
    return (o.float() if out_fp32 else o), lse


def decode_plan(B: int, Hg: int, G: int, Rn: int, Tcap: int, fp8_head_dim: int = 0) -> int:
    """Column spans an automatic :func:`decode` launch takes on the current device; ``fp8_head_dim``: over
    an fp8 cache of that head dim (``plan_decode_fp8``)."""
    if fp8_head_dim:
        return int(_ext.ops().flash_decode_fp8_plan(int(B), int(Hg), int(G), int(Rn), int(fp8_head_dim), int(Tcap)))
    return int(_ext.ops().flash_decode_plan(int(B), int(Hg), int(G), int(Rn), int(Tcap)))


# ---- paged decode: a ragged batch against a pool of pages (csrc/flash_paged.hip, flash_paged8.hip) ---
PAGE_SIZES = (32, 64, 128, 256)
_POS_SHIFT = 1 << 30   # positions are documented to stay below this


def decode_paged_eligible(dtype: torch.dtype, D: int, Dv: int, G: int, Rn: int, page_size: int, cache_dtype=None) -> bool:
    """The paged decode kernel takes this call: :func:`decode_eligible`'s shapes (16-bit, one head dim of
    32 / 64 / 96 / 128, at most 64 rows per gathered head) over pages of 32, 64, 128 or 256 slots.  ``dtype`` is
    the rows'; ``cache_dtype`` ``torch.float8_e4m3fn`` asks for the fp8-pool kernel (csrc/flash_paged8.hip),
    which takes the same shapes."""
    return decode_eligible(dtype, D, Dv, G, Rn, cache_dtype) and int(page_size) in PAGE_SIZES


def decode_paged(rows: torch.Tensor, qpool: torch.Tensor, vpool: torch.Tensor, pool_pos: torch.Tensor,
                 table: torch.Tensor, npages: torch.Tensor, pos0: torch.Tensor, H: int, scale: float, window: int = 0,
                 Hg: Optional[int] = None, nsplit: int = 0, out_fp32: bool = False,
                 max_pages: Optional[int] = None, qscale: Optional[torch.Tensor] = None,
                 vscale: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """:func:`decode` for a ragged batch over a paged cache -> (out (B, Rn, H*D) in ``rows.dtype``, lse
    (B, H, Rn) fp32 natural log).

    ``rows`` (B, Rn, H*D): ``Rn`` new rows of each of ``B`` sequences.  ``qpool`` / ``vpool`` (P, S, Hg*D): a
    pool of ``P`` pages of ``S`` slots, unit inner stride and one slot stride (the two halves of one ``[q|v]``
    pool).  ``pool_pos`` (P, S) int32: the global position of each slot, -1 = empty.  ``table`` (B, maxp)
    int32: the page of each logical block of each sequence, -1 = a hole.  ``npages`` (B,) int32: the table
    entries in use.  ``pos0`` (B,) int32: the position of each sequence's first new row; negative = the
    sequence is inactive and its rows see nothing.  Positions stay below ``2**30``.

    A slot of one of sequence ``b``'s pages is visible to its row ``i`` iff ``0 <= pos <= pos0[b] + i`` and
    (``window == 0`` or ``pos > pos0[b] + i - window``): :func:`decode`'s rule per sequence.  Slot and page order
    are free.  A row that sees nothing (an inactive sequence, one without pages) comes out NaN with lse -inf.

    ``table``, ``npages`` and ``pos0`` are read by the kernel, on the device: the call never waits for them,
    and a captured launch serves the next step once they are updated in place.  A table entry outside
    ``[0, P)`` that is not -1 gives an unspecified result for its sequence, never an access outside the pool.
    ``nsplit``: column spans (0: ``plan_decode_paged`` of ``csrc/flash_plan.h``, over ``max_pages`` pages per
    sequence: the table's width, or a tighter bound the caller knows; it sizes the grid only).

    ``qscale`` / ``vscale`` (P, Hg, S) fp32, the two halves of one (P, 2*Hg, S) buffer: ``qpool`` / ``vpool`` are
    ``float8_e4m3fn`` and slot ``c`` of page ``p``, gathered head ``h`` stands for ``qscale[p, h, c] * qpool[p, c,
    h*D:(h+1)*D]`` (and likewise ``v``): the format of :class:`xdot.PagedAttnCache` with ``cache_dtype="fp8"``.
    Eligible calls run the paged fp8 sweep (csrc/flash_paged8.hip; ``plan_decode_paged_fp8``).

    Calls the kernel does not take (:func:`decode_paged_eligible`: fp32 rows, D > 128, Dv != D, more than 64
    rows per gathered head, another page size) stay on the device without a kernel of their own: the pages (and
    an fp8 pool's scales) are gathered into a dense (B, maxp*S, .) cache, every sequence's positions are shifted
    by ``2**30 - pos0[b]`` (visibility depends on ``pos - pos0[b]`` only) and :func:`decode` runs at ``pos0 =
    2**30``: over an fp8 pool that is its fp8 route, so more than 64 rows per gathered head reach
    csrc/flash_extend8.hip.  CPU tensors and ``backend='torch'`` run ``xdot.parallel._ref.decode_paged``."""
    from ..parallel import _ref  # (xdot.parallel imports this module)

    B, Rn, C = rows.shape
    hg = int(Hg) if Hg else int(H)
    D, Dv, window = C // H, vpool.shape[-1] // hg, int(window or 0)
    fp8 = qscale is not None or vscale is not None
    if fp8 and not (qscale is not None and vscale is not None and qpool.dtype == vpool.dtype == torch.float8_e4m3fn):
        raise ValueError("flash.decode_paged: qscale and vscale go together, with float8_e4m3fn qpool and vpool")
    if not _ext.use_hip(rows, qpool, vpool):
        o, lse = _ref.decode_paged(rows, qpool, vpool, pool_pos, table, npages, pos0, int(H), float(scale), window, Hg,
                                   qscale, vscale)
        return (o if out_fp32 else o.to(rows.dtype)), lse
    if decode_paged_eligible(rows.dtype, D, Dv, H // hg, Rn, qpool.shape[1], torch.float8_e4m3fn if fp8 else None):
        if fp8:
            return _ext.ops().flash_decode_paged_fp8(rows.contiguous(), qpool, vpool, qscale, vscale, pool_pos, table, npages,
                                                     pos0, window, int(H), float(scale), hg, int(nsplit), bool(out_fp32),
                                                     int(max_pages or 0))
        return _ext.ops().flash_decode_paged(rows.contiguous(), qpool, vpool, pool_pos, table, npages, pos0, window, int(H),
                                             float(scale), hg, int(nsplit), bool(out_fp32), int(max_pages or 0))
    return _decode_paged_gathered(rows, qpool, vpool, pool_pos, table, npages, pos0, H, scale, window, Hg, nsplit, out_fp32,
                                  qscale, vscale)


def _decode_paged_gathered(rows, qpool, vpool, pool_pos, table, npages, pos0, H, scale, window=0, Hg=None, nsplit=0,
                           out_fp32=False, qscale=None, vscale=None):
    """:func:`decode_paged` without its kernel: gather to a dense cache (an fp8 pool to a dense fp8 cache, bytes
    and scales), shift the positions, :func:`decode`."""
    from ..parallel import _ref

    qc, vc, pos, *sc = _ref.paged_gather(qpool, vpool, pool_pos, table, npages, qscale, vscale)
    p0 = pos0.to(torch.int64).view(-1, 1)
    pos = torch.where((pos >= 0) & (p0 >= 0), pos + (_POS_SHIFT - p0), pos.new_full((), -1)).to(torch.int32)
    return decode(rows, qc, vc, pos, _POS_SHIFT, H, scale, window, Hg, nsplit, out_fp32, *sc)


def decode_paged_plan(B: int, Hg: int, G: int, Rn: int, max_pages: int, page_size: int, fp8_head_dim: int = 0) -> int:
    """Column spans an automatic :func:`decode_paged` launch takes on the current device; ``fp8_head_dim``: over
    an fp8 pool of that head dim (``plan_decode_paged_fp8``)."""
    if fp8_head_dim:
        return int(_ext.ops().flash_decode_paged_fp8_plan(int(B), int(Hg), int(G), int(Rn), int(fp8_head_dim), int(max_pages),
                                                          int(page_size)))
    return int(_ext.ops().flash_decode_paged_plan(int(B), int(Hg), int(G), int(Rn), int(max_pages), int(page_size)))


# ---- chunked prefill: many new rows against one rank's cache (csrc/flash_extend.hip) ---------------
EXTEND_MAX_GROUP = 128   # row heads per gathered head: one new row of a group fits the smallest row block
_EXTEND_MAX_NEW_ROWS = {96: 128}   # head dim -> the most new rows the kernel won the A/B at (profiles/extend.md)


def extend_eligible(dtype: torch.dtype, D: int, Dv: int, G: int, Rn: int, cache_dtype=None) -> bool:
    """The row-blocked kernel takes this call: 16-bit, one head dim of 32 / 64 / 96 / 128 for q and v, more
    than 64 rows (``G`` row heads x ``Rn`` new rows) per gathered head, where :func:`decode_eligible` ends,
    at most 128 row heads per gathered head, and a cache in the rows' dtype (``cache_dtype`` ``None``: the
    same).  An fp8 cache with that many rows has a kernel of its own (:func:`extend_fp8_eligible`).  Routed
    away: D = 96 with more than 128 new rows, where the forward kernels over an already packed mask were
    measured faster (profiles/extend.md; the other head dims were not measured and keep the kernel)."""
    if cache_dtype not in (None, dtype):
        return False
    return (dtype in (torch.bfloat16, torch.float16) and D == Dv and D in (32, 64, 96, 128)
            and G * Rn > DECODE_MAX_ROWS and 1 <= G <= EXTEND_MAX_GROUP and Rn <= _EXTEND_MAX_NEW_ROWS.get(D, Rn))


def extend_fp8_eligible(dtype: torch.dtype, D: int, Dv: int, G: int, Rn: int) -> bool:
    """The row-blocked fp8-cache kernel (csrc/flash_extend8.hip) takes this call: 16-bit rows over a
    ``float8_e4m3fn`` cache with per-slot scales, one head dim of 32 / 64 / 96 / 128 for q and v, more than 64
    rows (``G`` row heads x ``Rn`` new rows) per gathered head, where :func:`decode_eligible` ends, and at most
    128 row heads per gathered head.  The route it replaces dequantises the whole cache into fp32 per call;
    the kernel was 3.6x-12x faster than it at every measured shape (D = 96, 72 to 1024 new rows,
    profiles/extend_fp8.md), so no row count is routed away: the 16-bit kernel's D = 96 limit was set against
    the 16-bit forward kernels and does not carry over."""
    return (dtype in (torch.bfloat16, torch.float16) and D == Dv and D in (32, 64, 96, 128)
            and G * Rn > DECODE_MAX_ROWS and 1 <= G <= EXTEND_MAX_GROUP)


def extend(rows: torch.Tensor, qc: torch.Tensor, vc: torch.Tensor, col_pos: torch.Tensor, pos0: int, H: int,
           scale: float, window: int = 0, Hg: Optional[int] = None, nsplit: int = 0,
           out_fp32: bool = False, qscale: Optional[torch.Tensor] = None,
           vscale: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """:func:`decode` for more than 64 rows per gathered head, on the kernel alone: same arguments, same
    visibility rule from ``col_pos``, same outputs (a row that sees nothing: NaN, lse -inf), no mask and no
    ``Rn x Tcap`` tensor.  Workgroups take blocks of consecutive new rows (x the ``G`` row heads of a group)
    and sweep the cache through LDS, skipping tiles no row of the block can see.  ``nsplit``: column spans
    (0: ``plan_extend`` of ``csrc/flash_plan.h``; one span writes ``out`` directly).  ``qscale`` / ``vscale``
    (B, Hg, Tcap) fp32: ``qc`` / ``vc`` are ``float8_e4m3fn`` in :func:`decode`'s fp8 format and the call is
    the fp8 kernel's (csrc/flash_extend8.hip, :func:`extend_fp8_eligible`).  Raises on a call that is not
    eligible for its kernel or not on the GPU."""
    B, Rn, C = rows.shape
    hg = int(Hg) if Hg else int(H)
    D, Dv = C // H, vc.shape[-1] // hg
    if qscale is not None or vscale is not None:
        if not (qscale is not None and vscale is not None and qc.dtype == vc.dtype == torch.float8_e4m3fn
                and _ext.use_hip(rows, qc, vc) and extend_fp8_eligible(rows.dtype, D, Dv, H // hg, Rn)):
            raise ValueError(f"flash.extend: not a call of the fp8 kernel (dtype {rows.dtype}, cache {qc.dtype} / {vc.dtype} "
                             f"with both scales, head dims ({D}, {Dv}), G = {H // hg}, Rn = {Rn}, device {rows.device}); "
                             "flash.decode routes it")
        return _ext.ops().flash_extend_fp8(rows.contiguous(), _kv(qc), _kv(vc), qscale, vscale, col_pos, int(pos0),
                                           int(window or 0), int(H), float(scale), hg, int(nsplit), bool(out_fp32))
    if not (_ext.use_hip(rows, qc, vc) and extend_eligible(rows.dtype, D, Dv, H // hg, Rn, qc.dtype)):
        raise ValueError(f"flash.extend: not a call of the kernel (dtype {rows.dtype}, cache {qc.dtype}, head dims "
                         f"({D}, {Dv}), G = {H // hg}, Rn = {Rn}, device {rows.device}); flash.decode routes it")
    return _ext.ops().flash_extend(rows.contiguous(), _kv(qc), _kv(vc), col_pos, int(pos0), int(window or 0), int(H),
                                   float(scale), hg, int(nsplit), bool(out_fp32))


def extend_plan(B: int, Hg: int, G: int, Rn: int, D: int, Tcap: int, fp8: bool = False) -> int:
    """Column spans an automatic :func:`extend` launch of head dim ``D`` takes on the current device; ``fp8``:
    over an fp8 cache (``plan_extend_fp8``)."""
    if fp8:
        return int(_ext.ops().flash_extend_fp8_plan(int(B), int(Hg), int(G), int(Rn), int(D), int(Tcap)))
    return int(_ext.ops().flash_extend_plan(int(B), int(Hg), int(G), int(Rn), int(D), int(Tcap)))


def bwd_delta(dout: torch.Tensor, out: torch.Tensor, H: int) -> torch.Tensor:
    """δ = rowsum(dO ⊙ O) per (b, h, row): fp32 (B, H, R)."""
    return _ext.ops().flash_bwd_delta(dout.contiguous(), out.contiguous(), int(H))


def bwd_prep(dout: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, H: int):
    """(δ, lse2): δ = rowsum(dO ⊙ O) and the log2-domain LSE, fp32 (B, H, R), in one launch."""
    return _ext.ops().flash_bwd_prep(dout.contiguous(), out.contiguous(), lse.contiguous(), int(H))


def bwd_cols(dout, rows, kc, vc, out, lse, mk: Optional[PackedMask], H: int, scale: float,
             delta: Optional[torch.Tensor] = None, fp32_out: bool = True, prescaled: bool = False,
             lse2: Optional[torch.Tensor] = None, fp32_mode: Optional[int] = None,
             sbuf: Optional[torch.Tensor] = None, dsbuf: Optional[torch.Tensor] = None, passes: int = 3,
             out_dkv: Optional[torch.Tensor] = None, Hg: Optional[int] = None):
    """Gathered-side grads -> (packed [d_kc | d_vc] (B, T, 2*Hg*D), delta (B, H, R)).

    ``delta`` (from :func:`bwd_delta`) is computed here when not given; with ``lse2`` too (both
    from :func:`bwd_prep`) no prep pass is launched here.  The grads are fp32
    (``fp32_out``) or rounded once to the input dtype in the kernel epilogue.  ``sbuf``: the
    forward's :func:`score_buffer`; S is read from it and, without ``dsbuf``, it is OVERWRITTEN
    with dS for :func:`bwd_rows` (run once per forward).  ``dsbuf`` (:func:`score_buffers`): dS
    goes there instead; then ``passes`` may run one pass per call (2 = dQ, which writes dS; 1 = dV)
    with ``out_dkv`` = the first call's output, completed in place."""
    bits, flags = (mk.bits_t, mk.flags) if mk is not None else (None, None)
    return _ext.ops().flash_bwd_cols(dout.contiguous(), rows.contiguous(), _kv(kc), _kv(vc),
                                     out.contiguous(), lse.contiguous(), bits, flags, int(H), float(scale), delta,
                                     bool(fp32_out), bool(prescaled), lse2,
                                     fp32_code(rows.dtype) if fp32_mode is None else int(fp32_mode), sbuf, dsbuf,
                                     int(passes), out_dkv, *_hg(Hg))


def bwd_rows(dout, rows, kc, vc, lse, delta, mk: Optional[PackedMask], H: int, scale: float, nsplit: int = 0,
             prescaled: bool = False, fp32_mode: Optional[int] = None, sbuf: Optional[torch.Tensor] = None,
             dsbuf: Optional[torch.Tensor] = None, Hg: Optional[int] = None):
    """Row-side grad (B, R, H*D) in rows.dtype.  ``nsplit`` 0: the launcher's occupancy model
    (column splits so the row kernel fills the GPU; 1 measured 7 % / 32 % slower at N = 1 / 8).
    ``sbuf``: the score buffer after :func:`bwd_cols` wrote dS into it (dK is then its only product);
    with ``dsbuf`` dS is read from there."""
    bits, flags = _mask_args(mk)
    return _ext.ops().flash_bwd_rows(dout.contiguous(), rows.contiguous(), _kv(kc), _kv(vc),
                                     lse.contiguous(), delta.contiguous(), bits, flags, int(H), float(scale),
                                     int(nsplit), bool(prescaled),
                                     fp32_code(rows.dtype) if fp32_mode is None else int(fp32_mode), sbuf, dsbuf,
                                     *_hg(Hg))


def bwd(dout: torch.Tensor, rows: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, out: torch.Tensor,
        lse: torch.Tensor, mk: Optional[PackedMask], H: int, scale: float, prescaled: bool = False,
        fp32_mode: Optional[int] = None, sbuf: Optional[torch.Tensor] = None, Hg: Optional[int] = None):
    """-> (d_rows (B, R, H*D) rows.dtype, d_kc, d_vc (B, T, Hg*D) fp32 partial grads).

    ``prescaled``: ``rows`` is :func:`prescale` output (the buffer the forward read); d_rows is
    still the gradient of the unscaled rows.  ``sbuf``: the forward's score buffer (consumed)."""
    dkv, delta = bwd_cols(dout, rows, kc, vc, out, lse, mk, H, scale, prescaled=prescaled, fp32_mode=fp32_mode,
                          sbuf=sbuf, Hg=Hg)
    drows = bwd_rows(dout, rows, kc, vc, lse, delta, mk, H, scale, prescaled=prescaled, fp32_mode=fp32_mode,
                     sbuf=sbuf, Hg=Hg)
    Cg = (Hg or H) * (rows.shape[-1] // H)
    return drows, dkv[..., :Cg], dkv[..., Cg:]


# ---- attention sinks (csrc/sink.hip) -------------------------------------------------------------
def _sinks(sinks: torch.Tensor) -> torch.Tensor:
    """The logits as the kernels read them: contiguous fp32 / bf16 / fp16 (anything else -> fp32)."""
    s = sinks.detach()
    if s.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        s = s.float()
    return s.contiguous()


def sink_fold(out: torch.Tensor, lse: torch.Tensor, sinks: torch.Tensor, H: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fold one sink logit per head (``sinks`` (H,), fp32 / bf16 / fp16, not scaled by ``1/sqrt(d)``)
    into a finished forward, IN PLACE -> the same ``(out, lse)``: ``lse' = logaddexp(lse, s_h)``,
    ``out' = sigmoid(lse - s_h) * out``.  A fully masked row (``lse = -inf``, NaN in ``out``) comes
    out 0 with ``lse' = s_h``; ``s_h = -inf`` leaves the head as it is, bit for bit.  One launch."""
    _ext.ops().sink_fold(out, lse, _sinks(sinks), int(H))
    return out, lse


def sink_grad(delta: torch.Tensor, lse: torch.Tensor, sinks: torch.Tensor) -> torch.Tensor:
    """``ds`` (H,) fp32 ``= -sum_{b,r} exp(s_h - lse') * delta`` from the folded ``lse'`` and the δ of
    the folded output (both fp32 (B, H, R)): an ordered sum, bitwise reproducible.  Two launches."""
    return _ext.ops().sink_grad(delta.contiguous(), lse.contiguous(), _sinks(sinks))


# ---- launches into partial slots (gather chunks, ring blocks) ------------------------------------
def splits(B: int, R: int, T: int, H: int, rows_kernel: bool = False) -> int:
    """Partial slots one :func:`fwd_partial` (``rows_kernel``: :func:`bwd_rows_partial`) launch over
    ``T`` columns fills: the column splits the launcher picks for it."""
    return int(_ext.ops().flash_splits(int(B), int(R), int(T), int(H), bool(rows_kernel)))


def fwd_partial(rows: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, mk: Optional[PackedMask], H: int,
                scale: float, opart: torch.Tensor, lpart: torch.Tensor, slot: int, nsplit: int,
                prescaled: bool = False, fp32_mode: int = 0, Hg: Optional[int] = None) -> None:
    """Forward over one column segment into slots ``[slot, slot + nsplit)`` of ``opart`` (S, B, R, C)
    / ``lpart`` (S, B, H, R), fp32: per slot the output normalised over its columns and their LSE
    (-inf where they are all masked: the merges leave such a slot's output out).  ``rows`` contiguous."""
    bits, flags = _mask_args(mk)
    _ext.ops().flash_fwd_partial(rows, _kv(kc), _kv(vc), bits, flags, int(H), float(scale), opart, lpart, int(slot),
                                 int(nsplit), bool(prescaled), int(fp32_mode), *_hg(Hg))


def fwd_combine(opart: torch.Tensor, lpart: torch.Tensor, H: int, like: torch.Tensor):
    """Merge ALL slots -> (out like ``like`` (B, R, C), lse (B, H, R) fp32)."""
    return _ext.ops().flash_fwd_combine(opart, lpart, int(H), like)


def fwd_merge(opart: torch.Tensor, lpart: torch.Tensor, lrun: torch.Tensor, H: int) -> None:
    """Merge all slots into slot 0 of ``opart`` in fp32, in place; the merged LSE goes to ``lrun``
    (B, H, R) (slot 0 of ``lpart`` is still being read): the caller copies it back."""
    _ext.ops().flash_fwd_merge(opart, lpart, lrun, int(H))


def bwd_rows_partial(dout, rows, kc, vc, lse, delta, mk: Optional[PackedMask], H: int, scale: float,
                     dpart: torch.Tensor, slot: int, nsplit: int, prescaled: bool = False, fp32_mode: int = 0,
                     Hg: Optional[int] = None) -> None:
    """Row-side grads of one column segment into slots ``[slot, slot + nsplit)`` of ``dpart``
    (S, B, R, C) fp32.  ``dout`` / ``rows`` / ``lse`` / ``delta`` contiguous."""
    bits, flags = _mask_args(mk)
    _ext.ops().flash_bwd_rows_partial(dout, rows, _kv(kc), _kv(vc), lse, delta, bits, flags, int(H), float(scale),
                                      dpart, int(slot), int(nsplit), bool(prescaled), int(fp32_mode), *_hg(Hg))


def bwd_rows_sum(dpart: torch.Tensor, H: int, like: torch.Tensor) -> torch.Tensor:
    """Σ of all ``dpart`` slots -> (B, R, C) like ``like``."""
    return _ext.ops().flash_bwd_rows_sum(dpart, int(H), like)
