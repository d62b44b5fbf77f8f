"""fp64 references, rounding models and a torch emulation for the small kernels around the flash and
GEMM paths: the fused scale + mask + softmax (csrc/softmax.hip), the multi-tensor AdamW
(csrc/optim.hip), and the partial sums, prescale and MSE loss of csrc/reduce.hip.

tests/test_elementwise.py (CPU) shows that the emulation of the kernels' algorithm stays within the
bounds defined here and that eight wrong algorithms do not; tests/test_elementwise_gpu.py and three
tests of tests/test_kernels_gpu.py apply the same bounds to the kernels.  Every bound is F (= 2) times
a first-order model of the kernel's roundings (the "unit bound"); the tests print the worst ratio of
|error| to the unit bound (``RATIO`` lines, ``pytest -s``), listed at MEASURED below.

Every reference is computed in fp64 from the values the kernel reads: the 16-bit / fp32 tensors as
stored, and ``scale`` / the optimizer's hyper-parameters rounded to fp32, as the launch structs hold
them.

Not collected as a test (no ``test_`` prefix).
"""
import math
from types import SimpleNamespace

import torch

F32, BF16, FP16 = torch.float32, torch.bfloat16, torch.float16
DT_IDS = {F32: "fp32", BF16: "bf16", FP16: "fp16"}
DTYPES = (F32, BF16, FP16)
NEG_INF = -float("inf")

F = 2.0                      # asserted factor on every unit bound
U32 = 2.0 ** -24             # half an ulp of 1 in fp32
# one rounding to the output dtype, relative (half an ulp of 1; 0 for fp32: the fp32 terms carry it)
EPS_OUT = {F32: 0.0, BF16: 2.0 ** -9, FP16: 2.0 ** -11}
# What a correct algorithm is held to in units of the unit bound (tests/test_elementwise.py).  The
# bf16 figure above (the one tests/_flash_profiles.py uses) is half the largest relative error of one
# bf16 rounding, 2^-8 / (1 + 2^-8) just above a power of two (8 significand bits); fp16's 2^-11 is
# the whole of it.  One correct rounding to bf16 alone therefore reaches 1.99 of the unit bound, and
# F = 2 leaves the fp32 terms of the bound, but nothing else, on top of it.
EMU_LIMIT = {F32: 1.0, BF16: F, FP16: 1.0}
# the absolute rounding error below the normal range of the output dtype
TINY = {F32: 2.0 ** -125, BF16: 2.0 ** -125, FP16: 2.0 ** -24}
# half an ulp of 1 of the parameter dtype (AdamW writes the parameter in its own dtype)
U_P = {F32: 2.0 ** -24, BF16: 2.0 ** -9, FP16: 2.0 ** -11}

# MEASURED (worst ratio of |error| to the unit bound, i.e. with F = 1, over every case of
# tests/test_elementwise_gpu.py and the three tests of tests/test_kernels_gpu.py that use these bounds;
# asserted: <= F = 2, the fp32 moments <= 1).  "emulation" is the torch emulation in this file on the
# same cases (tests/test_elementwise.py).
#   softmax forward, elements / row sums:
#     emulation:  fp32 1.00 / 0.24 (amplitude 60: 1.11 / 0.03)   bf16 1.99 / 1.41   fp16 0.97 / 0.61
#     MI355X:     fp32 1.12 / 0.24 (amplitude 60: 1.25 / 0.03)   bf16 1.99 / 1.41   fp16 0.97 / 0.61
#   softmax backward:
#     emulation:  fp32 0.38   bf16 1.99   fp16 0.92
#     MI355X:     fp32 0.38   bf16 1.99   fp16 0.94      (T = 131080, rows past element 2^31: bf16 1.99 / 1.99)
#   AdamW, one step, parameter / exp_avg / exp_avg_sq:
#     emulation:  fp32 1.25 / 0.49 / 0.66   bf16 1.99 / 0.47 / 0.49   fp16 0.99 / 0.47 / 0.64
#     MI355X:     fp32 1.18 / 0.47 / 0.65   bf16 1.99 / 0.47 / 0.65   fp16 1.00 / 0.47 / 0.65
#   AdamW, three-step runs (ratio to the run's bound / F):
#     MI355X:     fp32 0.09   bf16 0.52   fp16 0.99;  tests/test_kernels_gpu.py (randn parameters, betas
#                 (0.9, 0.95), weight decay 0.05): fp32 1.94 (the emulation gives the same 1.94)   bf16 0.70
#   MSE loss (ratio to the worst-case summation bound):  fp32 0.01   bf16 0.73   fp16 0.05
# The bf16 figures are one rounding to bf16 (EMU_LIMIT above); everything else is the fp32 model.
# fp32 forward at amplitude 60: three roundings grow with |s_i - max| (the subtraction, the product
# with log2 e, and log2 e's own rounding, 0.22 u32), against the 2 u32 |s_i - max| of the unit bound;
# an element 80 nats under its row's max with a small |s_i| exceeds the unit bound by up to a tenth
# in the emulation, and the kernel's v_exp_f32 (1 ulp) adds to that.  F = 2 covers both.
# The bias-correction term of the AdamW bound stays: the kernel and its launch code are unchanged.


def f32(x: float) -> float:
    """``x`` rounded to fp32, as a Python float: what a ``float`` field of a launch struct holds."""
    return torch.tensor(float(x), dtype=torch.float32).item()


LOG2E_F32 = f32(1.4426950408889634)


# ---- softmax: dispatch table (csrc/softmax.hip fwd_dispatch / bwd_dispatch) ---------------------------
# (largest T, BLOCK, NPT): a thread holds NPT groups of 8 consecutive elements, group n of thread t
# starts at (n * BLOCK + t) * 8; longer rows stream with BLOCK = 1024 and ceil(T / 8192) groups
DISPATCH = ((2048, 256, 1), (4096, 256, 2), (8192, 1024, 1), (16384, 1024, 2), (32768, 1024, 4), (65536, 1024, 8))
BRANCHES = ("256x1", "256x2", "1024x1", "1024x2", "1024x4", "1024x8", "stream")
# the edges of each branch, a full-vector tail and a ragged tail
BRANCH_T = {"256x1": (1, 7, 8, 9, 2047, 2048), "256x2": (2049, 2056, 4096), "1024x1": (4097, 4104, 8192),
            "1024x2": (8200, 12289, 16384), "1024x4": (16392, 20001, 32768), "1024x8": (32776, 50001, 65536),
            "stream": (65537, 65544, 70000)}
# one vector (T % 8 == 0) and one odd T per branch for the mask forms, views and special rows
EDGE_T = {"256x1": (2048, 2047), "256x2": (4096, 4095), "1024x1": (8192, 8191), "1024x2": (16384, 16383),
          "1024x4": (32768, 32767), "1024x8": (65536, 65535), "stream": (65544, 65545)}
SHAPE = (2, 2, 3)            # (B, H, R): 12 rows, two batches, so the mask row map's quotient is not always 0
SCALE = 0.37


def branch_of(T: int):
    """-> (name, BLOCK, NPT or None for the stream kernels, groups per thread)."""
    for tmax, block, npt in DISPATCH:
        if T <= tmax:
            return f"{block}x{npt}", block, npt, npt
    return "stream", 1024, None, -(-T // 8192)


def case_id(T: int) -> str:
    return f"{branch_of(T)[0]}-T{T}-{'vec' if T % 8 == 0 else 'odd'}"


ALL_T = [T for b in BRANCHES for T in BRANCH_T[b]]
EDGE_CASES = [T for b in BRANCHES for T in EDGE_T[b]]
assert all(branch_of(T)[0] == b for b in BRANCHES for T in BRANCH_T[b] + EDGE_T[b])


def bwd_chain(T: int) -> int:
    """K of the backward bound: the longest sequential fp32 add chain of the row dot product: 8
    elements per group and thread (8 NPT; 8 ceil(T / 8192) in the stream kernel), the 6 levels of the
    wave butterfly and the BLOCK / 64 wave sums added in order."""
    _, block, _, groups = branch_of(T)
    return 8 * groups + 6 + block // 64


def make_scores(T, dtype, amp=3.0, seed=0, shape=SHAPE, hidden_lift=0.0):
    """-> (x (B, H, R, T) in ``dtype``, mask (B, R, T) bool with 30 % hidden) on the CPU.  Column 0 of
    every row stays live.  ``hidden_lift``: added to the hidden entries of x, so that a maximum taken
    before masking sits that far above every live score."""
    B, H, R = shape
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + T)
    x = torch.randn(B, H, R, T, generator=g) * amp
    mask = torch.rand(B, R, T, generator=g) < 0.3
    mask[..., 0] = False
    if hidden_lift:
        x = x + hidden_lift * mask.unsqueeze(1)
    return x.to(dtype), mask


def make_dy(x, seed=0):
    g = torch.Generator(device="cpu").manual_seed(77 + 1000 * seed + x.shape[-1])
    return torch.randn(x.shape, generator=g).to(x.dtype)


# ---- softmax: mask row map ----------------------------------------------------------------------------
def mask_row_index(rows: int, mdiv: int, mmul: int, mmod: int, bug=None) -> torch.Tensor:
    """The mask row of each score row, as csrc/softmax.hip computes it.  ``bug='mask_no_batch'``: the
    quotient term dropped."""
    r = torch.arange(rows)
    if bug == "mask_no_batch":
        return r % mmod
    return (r // mdiv) * mmul + r % mmod


def broadcast_mask(x: torch.Tensor, mask):
    """What torch broadcasting makes of the mask: (B, R, T) over the heads of (B, H, R, T) scores,
    (B, 1, R, T), or the scores' own shape.  -> bool tensor of x's shape, or None."""
    if mask is None:
        return None
    if mask.dim() == 3 and x.dim() == 4:
        mask = mask.unsqueeze(1)
    return mask.expand(x.shape)


# ---- softmax: fp64 references and bounds --------------------------------------------------------------
def softmax_ref(x, mask, scale):
    """-> (softmax in fp64 (NaN on a row with no live entry, as torch.softmax), the masked scores in
    nats).  ``mask``: anything :func:`broadcast_mask` takes."""
    s = x.double() * f32(scale)
    m = broadcast_mask(x, mask)
    if m is not None:
        s = s.masked_fill(m, NEG_INF)
    return torch.softmax(s, -1), s


def softmax_fwd_ratios(y, x, mask, scale):
    """Ratios to the unit bound of the forward,
        |y - ref| <= u32 (8 + 2 (|s_i| + |s_i - max|)) ref + eps_out ref + TINY
    (the scale multiply and the subtraction round relative to |s_i| and |s_i - max|, the argument
    reduction of exp multiplies |s_i - max| by a rounded log2 e, and exp, the sum, the reciprocal and
    the product round a few times more), and of the row sums, |sum_i y_i - 1| <= sum_i (bound_i).
    Rows whose reference is NaN (no live entry) must be NaN and nothing else may be; entries whose
    reference is exactly 0 (hidden, or -inf in x) must be exactly 0.  A violation of those gives inf.
    -> dict(fwd=, rowsum=)."""
    ref, s = softmax_ref(x, mask, scale)
    yd = y.double()
    dead = torch.isnan(ref).all(-1, keepdim=True)
    assert not (torch.isnan(ref) & ~dead).any()
    if not torch.equal(torch.isnan(yd), dead.expand(yd.shape)):
        return {"fwd": float("inf"), "rowsum": float("inf")}
    zero = (ref == 0) & torch.isinf(s)
    if (yd[zero] != 0).any():
        return {"fwd": float("inf"), "rowsum": float("inf")}
    live = ~dead.squeeze(-1)
    ref, s, yd = ref[live], s[live], yd[live]
    if ref.numel() == 0:
        return {"fwd": 0.0, "rowsum": 0.0}
    mx = s.amax(-1, keepdim=True)
    sf = torch.where(torch.isinf(s), torch.zeros_like(s), s)       # (ref is 0 there)
    unit = U32 * (8.0 + 2.0 * (sf.abs() + (sf - mx).abs())) * ref + EPS_OUT[y.dtype] * ref + TINY[y.dtype]
    return {"fwd": ((yd - ref).abs() / unit).max().item(),
            "rowsum": ((yd.sum(-1) - 1.0).abs() / unit.sum(-1)).max().item()}


def softmax_bwd_ref(y, dy, scale):
    """``scale * y * (dy - sum_j y_j dy_j)`` in fp64 from the ``y`` the kernel is handed.
    -> (dx, dy - dot, sum_j |y_j dy_j|)."""
    yd, dd = y.double(), dy.double()
    dot = (yd * dd).sum(-1, keepdim=True)
    return f32(scale) * yd * (dd - dot), dd - dot, (yd * dd).abs().sum(-1, keepdim=True)


def softmax_bwd_ratios(dx, y, dy, scale):
    """Ratio to the unit bound of the backward,
        |dx - ref| <= u32 |scale| y_i (4 |dy_i - dot| + K sum_j |y_j dy_j|) + eps_out |ref| + TINY,
    K = :func:`bwd_chain`: the fp32 dot is off by at most K u32 sum_j |y_j dy_j|, and the subtraction
    and the two products round relative to the result.  -> dict(bwd=)."""
    ref, diff, absdot = softmax_bwd_ref(y, dy, scale)
    K = bwd_chain(y.shape[-1])
    unit = U32 * abs(f32(scale)) * y.double() * (4.0 * diff.abs() + K * absdot) + EPS_OUT[y.dtype] * ref.abs() \
        + TINY[y.dtype]
    d = dx.double()
    if not torch.isfinite(d).all():
        return {"bwd": float("inf")}
    return {"bwd": ((d - ref).abs() / unit).max().item()}


def assert_ratios(what, ratios, limit=F):
    bad = {k: v for k, v in ratios.items() if not v <= limit}
    assert not bad, f"{what}: ratio to the unit bound above {limit}: {bad}  [all {ratios}]"
    return ratios


# ---- softmax: torch emulation of the kernels' algorithm (CPU) ------------------------------------------
FWD_BUGS = ("tail_zero", "max_before_mask", "stream_no_factor")


def _exp(d):
    """``__expf``: exp2 of the argument times an fp32 log2 e."""
    return torch.exp2(d * LOG2E_F32)


def _block_sum(th):
    """block_reduce of (rows, BLOCK) thread values: xor butterfly inside each 64-lane wave (offsets
    32 .. 1), then the wave sums added in wave order."""
    rows, block = th.shape
    w = th.view(rows, block // 64, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ o]
    r = w[:, 0, 0]
    for i in range(1, block // 64):
        r = r + w[:, i, 0]
    return r


def _groups(a, T, block, groups, fill):
    """(rows, T) -> (rows, groups, BLOCK, 8): element i of group n of thread t is column (n BLOCK + t) 8 + i."""
    rows = a.shape[0]
    pad = torch.full((rows, groups * block * 8 - T), fill, dtype=a.dtype)
    return torch.cat([a, pad], 1).view(rows, groups, block, 8)


def emulate_softmax_fwd(x, mask, scale, bug=None, map_bug=None):
    """fp32 emulation of fwd_cached / fwd_stream in the kernels' order: scale multiply, mask and tail
    -> -inf, row max, exp2((s - max) log2 e), per-thread sums over 8-element groups strided by the
    block, wave butterfly, waves in order, one reciprocal, the output rounded to x's dtype.

    ``mask``: (B, R, T) for (B, H, R, T) scores, read through the kernel's row map.  ``bug``: one of
    FWD_BUGS; ``map_bug='mask_no_batch'``: see :func:`mask_row_index`."""
    T = x.shape[-1]
    x2 = x.reshape(-1, T)
    rows = x2.shape[0]
    _, block, npt, groups = branch_of(T)
    s = x2.float() * torch.tensor(scale, dtype=torch.float32)
    live = s
    if mask is not None:
        B, H, R, _ = x.shape
        idx = mask_row_index(rows, H * R, R, R, map_bug)
        live = s.masked_fill(mask.reshape(-1, T)[idx], NEG_INF)
    fill = 0.0 if bug == "tail_zero" else NEG_INF
    v = _groups(live, T, block, groups, fill)
    vmax = _groups(s, T, block, groups, fill) if bug == "max_before_mask" else v
    if npt is not None:
        mx = vmax.amax((1, 2, 3))
        e = _exp(v - mx.view(-1, 1, 1, 1))
        th = torch.zeros(rows, block)
        for n in range(groups):
            for i in range(8):
                th = th + e[:, n, :, i]
        inv = 1.0 / _block_sum(th)
        y = e * inv.view(-1, 1, 1, 1)
    else:
        mt = torch.full((rows, block), NEG_INF)
        st = torch.zeros(rows, block)
        for n in range(groups):
            nm = torch.maximum(mt, vmax[:, n].amax(-1))
            upd = nm != NEG_INF
            safe = torch.where(upd, nm, torch.zeros_like(nm))
            sn = st * _exp(mt - safe)
            for i in range(8):
                sn = sn + _exp(v[:, n, :, i] - safe)
            st = torch.where(upd, sn, st)
            mt = torch.where(upd, nm, mt)
        gmx = mt.amax(-1, keepdim=True)
        part = st if bug == "stream_no_factor" else st * _exp(mt - gmx)
        part = torch.where(mt == NEG_INF, torch.zeros_like(part), part)
        inv = 1.0 / _block_sum(part)
        y = _exp(v - gmx.view(-1, 1, 1, 1)) * inv.view(-1, 1, 1, 1)
    return y.reshape(rows, -1)[:, :T].to(x.dtype).view(x.shape)


def emulate_softmax_bwd(y, dy, scale, bug=None):
    """fp32 emulation of bwd_cached / bwd_stream: per-thread dot over its groups, block sum,
    (scale * y) * (dy - dot) rounded to y's dtype.  ``bug='dot_misses_last_group'``: the dot leaves
    out every thread's last group (the last NPT chunk of the row)."""
    T = y.shape[-1]
    _, block, _, groups = branch_of(T)
    yv = _groups(y.reshape(-1, T).float(), T, block, groups, 0.0)
    dv = _groups(dy.reshape(-1, T).float(), T, block, groups, 0.0)
    th = torch.zeros(yv.shape[0], block)
    for n in range(groups - 1 if bug == "dot_misses_last_group" else groups):
        for i in range(8):
            th = th + yv[:, n, :, i] * dv[:, n, :, i]
    dot = _block_sum(th).view(-1, 1, 1, 1)
    dx = (torch.tensor(scale, dtype=torch.float32) * yv) * (dv - dot)
    return dx.reshape(yv.shape[0], -1)[:, :T].to(y.dtype).view(y.shape)


# ---- AdamW ----------------------------------------------------------------------------------------------
ADAM_LR = 3e-3
ADAM_BETAS = (0.9, 0.999)    # FusedAdamW's defaults
ADAM_EPS = 1e-8
ADAM_WD = 1e-2
ADAM_NUMELS = (1, 3, 4, 5, 1023, 1024, 1025, 4098, 768 * 768)   # around ADAM_BLOCK_ELEMS = 1024; 576 blocks
ADAM_BUGS = ("no_write", "no_wd", "bc_prev_step")
# Parameters are 0.02 * randn (the size of an initialised projection weight).  With randn parameters a
# bf16 ulp (4e-3 at 1) is as large as one update (lr = 3e-3) and no bound in ulps of the parameter
# can tell an update from none.
ADAM_P_STD = 0.02


def make_adam_state(numel, dtype, seed, g32=False):
    """-> ns(p in ``dtype``, g in ``dtype`` (fp32 if ``g32``), m, v fp32) on the CPU: nonzero moments."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    p = (ADAM_P_STD * torch.randn(numel, generator=gen)).to(dtype)
    g = torch.randn(numel, generator=gen)
    m = 0.1 * torch.randn(numel, generator=gen)
    v = 0.01 * torch.randn(numel, generator=gen) ** 2 + 1e-4
    return SimpleNamespace(p=p, g=g if g32 else g.to(dtype), m=m, v=v)


def adamw_ref(p, g, m, v, t, lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS, wd=ADAM_WD, device_state=False,
              torch_path=False):
    """One AdamW step in fp64 from the state the kernel reads.  lr, betas, eps and weight decay are
    the fp32 values of the launch struct and 1 - beta is ``1.f - beta`` (exact in fp32); the bias
    corrections 1 - beta^t are exact, from the betas the corrections are made of: the host's doubles,
    or with ``device_state`` (capturable) the kernel's fp32 betas.  ``torch_path``: the CPU update of
    FusedAdamW instead, whose torch ops take 1 - beta as the double rounded to fp32 (1.3e-5 from
    1.f - beta2 at the default beta2) and the other scalars as doubles.

    -> ns(p, m, v, delta (the Adam term of the update), delta_abs (the same with the magnitudes of the
    two terms of its numerator summed), bm, bv (the sums of magnitudes the moment bounds are made of), bc2)."""
    b1, b2 = f32(betas[0]), f32(betas[1])
    o1, o2 = (f32(1.0 - betas[0]), f32(1.0 - betas[1])) if torch_path else (1.0 - b1, 1.0 - b2)
    lr_, eps_, wd_ = (float(lr), float(eps), float(wd)) if torch_path else (f32(lr), f32(eps), f32(wd))
    gd = g.double()
    m2 = b1 * m.double() + o1 * gd
    v2 = b2 * v.double() + o2 * gd * gd
    bm = (b1 * m.double()).abs() + (o1 * gd).abs()
    c1, c2 = (b1, b2) if device_state else (float(betas[0]), float(betas[1]))
    bc1, bc2 = 1.0 - c1 ** t, 1.0 - c2 ** t
    per_m = (lr_ / bc1) / (v2.sqrt() / math.sqrt(bc2) + eps_)
    delta = -per_m * m2
    return SimpleNamespace(p=p.double() * (1.0 - lr_ * wd_) + delta, m=m2, v=v2, delta=delta, delta_abs=per_m * bm,
                           bm=bm, bv=(b2 * v.double()).abs() + (o2 * gd * gd).abs(), bc2=bc2)


def adamw_param_unit(ref, dtype):
    """u_p |ref| + TINY + u32 (8 + 1 / (1 - beta2^t)) |delta|: the rounding of the written parameter
    (below the normal range of the dtype an absolute one: fp16 parameters of 0.02 randn have such
    elements), the fp32 roundings of the Adam term, and the bias correction 1 - beta2^t computed in
    fp32 from a rounded beta2^t (absolute error u32, relative u32 / (1 - beta2^t): 6e-5 at t = 1).

    |delta| is ``delta_abs``: lr / bc1 * (|beta1 m| + |(1 - beta1) g|) / (sqrt(v / bc2) + eps).  Where
    beta1 m and (1 - beta1) g cancel, the new exp_avg carries the roundings of its two terms (the
    moment bound itself allows 4 u32 of their magnitudes) and the update inherits them, however small
    the update is.  Among 768 * 768 elements some cancel to 1e-5 of their terms: the emulation of a
    correct kernel is then 10 times past a bound made of the update's own magnitude (fp32, t = 1)."""
    return U_P[dtype] * ref.p.abs() + TINY[dtype] + U32 * (8.0 + 1.0 / ref.bc2) * ref.delta_abs


def adamw_ratios(p, m, v, ref):
    """Ratios to the unit bounds: the parameter (asserted <= F), and the fp32 moments
    |m - ref| <= 4 u32 (|beta1 m| + |(1 - beta1) g|), likewise v (asserted <= 1)."""
    if ref.p.numel() == 0:
        return {"p": 0.0, "m": 0.0, "v": 0.0}
    out = {"p": ((p.double() - ref.p).abs() / adamw_param_unit(ref, p.dtype)).max().item()}
    for k, got, want, b in (("m", m, ref.m, ref.bm), ("v", v, ref.v, ref.bv)):
        assert got.dtype == torch.float32
        out[k] = ((got.double() - want).abs() / (4.0 * U32 * b).clamp_min(1e-300)).max().item()
    return {k: (x if x == x else float("inf")) for k, x in out.items()}


def assert_adamw(what, p, m, v, ref):
    r = adamw_ratios(p, m, v, ref)
    assert_ratios(what, {"p": r["p"]}, F)
    assert_ratios(what, {"m": r["m"], "v": r["v"]}, 1.0)
    return r


def emulate_adamw(p, g, m, v, t, lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS, wd=ADAM_WD, bug=None):
    """fp32 emulation of adamw_kernel with the host's bias corrections (``1.f - (float)pow(beta, t)``).
    The final ``p * decay - step_size * m / (...)`` is one fused multiply-add (-ffp-contract=fast, the
    compiler's default for device code).  -> (p in its dtype, m, v fp32).  ``bug``: one of ADAM_BUGS."""
    t32 = lambda x: torch.tensor(x, dtype=torch.float32)
    b1, b2, lr_, eps_, wd_ = t32(betas[0]), t32(betas[1]), t32(lr), t32(eps), t32(wd)
    tb = t - 1 if bug == "bc_prev_step" else t
    bc1 = t32(1.0) - t32(float(betas[0]) ** tb)
    bc2_sqrt = torch.sqrt(t32(1.0) - t32(float(betas[1]) ** tb))
    gf = g.float()
    m2 = b1 * m + (1.0 - b1) * gf
    v2 = b2 * v + (1.0 - b2) * gf * gf
    step_size = lr_ / bc1
    decay = t32(1.0) if bug == "no_wd" else 1.0 - lr_ * wd_
    q = step_size * m2 / (torch.sqrt(v2) / bc2_sqrt + eps_)
    pn = (p.double() * decay.double() - q.double()).float().to(p.dtype)
    return (p.clone() if bug == "no_write" else pn), m2, v2


def adamw_run_ref(p0, grads, dtype, lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS, wd=ADAM_WD):
    """A run of len(grads) steps from zero moments in fp64, the parameter rounded to ``dtype`` after each
    step (moments stay fp64).  -> (final p in fp64, the element bound of the run).

    The bound is the sum of the one-step bounds along the run: per step F u_p |p_s| for the rounding
    of the written parameter (2 u_p |p| is one ulp: where the kernel's value and the reference's
    straddle a rounding boundary they part by one ulp, and the next step carries that on) plus the
    terms in |delta_s| of :func:`adamw_param_unit`.  For len(grads) = 3 and |p_s| = |p| that is
    3 F u_p |p|."""
    p = p0.to(dtype)
    m = torch.zeros(p.shape, dtype=torch.float64)
    v = torch.zeros(p.shape, dtype=torch.float64)
    bound = torch.zeros(p.shape, dtype=torch.float64)
    for t, g in enumerate(grads, 1):
        r = adamw_ref(p, g, m, v, t, lr, betas, eps, wd)
        p, m, v = r.p.to(dtype), r.m, r.v
        r.p = p.double()
        bound += F * adamw_param_unit(r, dtype)
    return p.double(), bound


def make_adam_run(dtype, numel=768 * 768, seed=11):
    """The three-step run: -> (p0 fp32, three gradients g, 2 g, 3 g in ``dtype``, the reference's final p,
    the element bound).  Every step moves every element by about lr in the same direction."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    p0 = ADAM_P_STD * torch.randn(numel, generator=gen)
    g0 = torch.randn(numel, generator=gen)
    grads = [(g0 * (s + 1)).to(dtype) for s in range(3)]
    want, bound = adamw_run_ref(p0, grads, dtype)
    return p0, grads, want, bound


# ---- partial sums, prescale, MSE -------------------------------------------------------------------------
def sum_partials_ref(part, dtype):
    """fp32 sum of the slots in slot order (``acc = part[0]; acc += part[s]``), rounded once."""
    acc = part[0].clone()
    for s in range(1, part.shape[0]):
        acc = acc + part[s]
    return acc.to(dtype)


def prescale_ref(x, scale):
    """``(x.float() * c2).to(dtype)``, ``c2 = float32(scale) * float32(log2 e)`` rounded to fp32."""
    c2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    return (x.float() * c2).to(x.dtype)


def mse_ref(y, t):
    """-> (loss in fp64, dy = ((y - t) * (2 / n)) in fp32 rounded to the dtype, the relative bound of the loss).

    Summation model of mse_fwd_kernel / mse_final_kernel for n <= 256 * 1024 vectors: every term is
    nonnegative, and a term passes through the rounding of y - t (counted twice: it is squared), V
    fused multiply-adds of its thread (V = 4 fp32 / 8 16-bit elements per vector), 6 butterfly levels
    and 2 adds of the workgroup, one add, 6 levels and 2 adds of the final kernel, the rounded 1 / n
    and the product with it: at most (V + 21) u32 relative, plus the rounding of the loss to its dtype."""
    n = y.numel()
    d = y.double() - t.double()
    g2 = torch.tensor(2.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    dy = ((y.float() - t.float()) * g2).to(y.dtype)
    V = 16 // y.element_size()
    assert n // V <= 256 * 1024
    return (d * d).sum().item() / n, dy, (V + 21) * U32 + (U32 if y.dtype == F32 else EPS_OUT[y.dtype])
