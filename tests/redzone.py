"""Guard-band buffers and per-element error bounds for the kernel edge tests (a helper module, not a conftest).

Guard bands.  ``guarded`` lays ONE flat allocation out as

    [front guard | payload, with the pad columns between `width` and `ld` of every row and the gap between
     `rows * ld` and `batch_stride` of every batch | back guard]

and fills everything that is not payload with a fixed quiet-NaN bit pattern.  ``assert_untouched`` compares those words as
integers afterwards (NaN != NaN does not matter), so a kernel that WRITES outside its stated extent is caught, named by
region.  The same constructor makes inputs: a kernel that READS a pad column, or the row after the last one, pulls a NaN
into some output, where the test's finite-ness check finds it.

    NOTE on ReLU: ``act = ReLU`` launders NaN - the kernels' ``v > 0.f ? v : 0.f`` gives 0 for a NaN - so a read of poison
    would go unseen behind it.  Read-poison cases therefore run with act none or SiLU; ReLU gets a value-only case.

Payloads of OUTPUT buffers start as a second NaN pattern (``UNWRITTEN``), so an element the kernel should have written
and did not fails the same finite-ness check.

Per-element bounds.  ``elementwise_bound(S, n) = n * 2**-24 * S``: S_i is the float64 sum of the absolute values of the
terms that form element i, n the number of fp32 roundings on the longest dependency path to it (for a reduction over k
terms: k plus the epilogue operations).  Derived from the format, never fitted to what a kernel returns.
"""
from __future__ import annotations

import torch

U = 2.0 ** -24  # one fp32 rounding (half an ulp, relative)
TINY = 2.0 ** -126  # smallest normal fp32: results below it may be flushed to zero by the transcendental unit
GUARD = 4096  # elements per guard (a multiple of 8 floats)
POISON32 = 0x7FC0DEAD  # quiet NaN (exponent all ones, quiet bit set), recognisable payload
POISON64 = 0x7FF8DEAD7FC0DEAD  # quiet NaN as a double; its two halves are fp32 quiet NaNs too
UNWRITTEN32 = 0x7FC0BEEF
UNWRITTEN64 = 0x7FF8BEEF7FC0BEEF

_INT = {4: torch.int32, 8: torch.int64}


def _signed(v, bits):
    return v - (1 << bits) if v >= (1 << (bits - 1)) else v


class Guarded:
    """a strided payload view [batch][rows][:width] inside one guarded flat allocation"""

    def __init__(self, flat, front, batch, rows, width, ld, batch_stride, pattern):
        self.flat, self.front = flat, front
        self.batch, self.rows, self.width, self.ld, self.batch_stride = batch, rows, width, ld, batch_stride
        self.pattern = pattern
        self.span = (batch - 1) * batch_stride + (rows - 1) * ld + width  # first payload word .. last payload word
        self.view = flat.as_strided((batch, rows, width), (batch_stride, ld, 1), front)

    @property
    def t(self):
        """[rows][:width] view of batch 0 (what the 2-D entry points take)"""
        return self.view[0]

    @property
    def bs(self):
        return self.batch_stride

    def fill(self, values):
        self.view.copy_(values.reshape(self.batch, self.rows, self.width).to(self.flat.dtype))
        return self

    def payload(self):
        """contiguous CPU copy [batch][rows][width]"""
        return self.view.detach().cpu().contiguous()

    def ints(self):
        return self.flat.detach().cpu().view(_INT[self.flat.element_size()])

    def payload_mask(self):
        m = torch.zeros(self.flat.numel(), dtype=torch.bool)
        m.as_strided((self.batch, self.rows, self.width), (self.batch_stride, self.ld, 1), self.front).fill_(True)
        return m

    def region_of(self, off):
        """name of the non-payload region holding flat offset `off`"""
        if off < self.front:
            return "front guard"
        rel = off - self.front
        if rel >= self.span:
            return "back guard"
        b, inb = divmod(rel, self.batch_stride)
        r, c = divmod(inb, self.ld)
        if r >= self.rows:
            return f"gap after batch {b}"
        return f"pad of row {r}" + (f" of batch {b}" if self.batch > 1 else "")


def guarded(shape_rows, width, ld=None, *, dtype=torch.float32, align_bytes=16, batch=1, batch_stride=None, poison=None,
            device="cuda", unwritten=True):
    """A `Guarded` whose payload start is `align_bytes`-aligned.  `poison`: the NaN bit pattern of guards, pads and gaps
    (default POISON32 / POISON64 by element size).  `unwritten`: start the payload as the UNWRITTEN NaN pattern."""
    rows = int(shape_rows)
    ld = width if ld is None else ld
    assert ld >= width >= 1 and rows >= 1 and batch >= 1
    batch_stride = rows * ld if batch_stride is None else batch_stride
    assert batch_stride >= rows * ld or batch == 1
    esz = torch.empty(0, dtype=dtype).element_size()
    pattern = poison if poison is not None else (POISON32 if esz == 4 else POISON64)
    span = (batch - 1) * batch_stride + (rows - 1) * ld + width
    slack = max(align_bytes // esz, 8)
    total = GUARD + slack + span + GUARD + 8
    flat = torch.empty(total, dtype=dtype, device=device)
    iv = flat.view(_INT[esz])
    iv.fill_(_signed(pattern, 8 * esz))
    front = GUARD
    while (flat.data_ptr() + front * esz) % align_bytes:
        front += 1
    assert front < GUARD + slack
    g = Guarded(flat, front, batch, rows, width, ld, batch_stride, pattern)
    if unwritten:
        un = UNWRITTEN32 if esz == 4 else UNWRITTEN64
        iv.as_strided((batch, rows, width), (batch_stride, ld, 1), front).fill_(_signed(un, 8 * esz))
    assert g.view.data_ptr() % align_bytes == 0
    return g


def assert_untouched(buf: Guarded, what=""):
    """every guard, pad and gap word of `buf` still holds the poison pattern, bit for bit"""
    iv = buf.ints()
    bad = (iv != _signed(buf.pattern, 8 * buf.flat.element_size())) & ~buf.payload_mask()
    if bad.any():
        off = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {buf.region_of(off)} overwritten: first offending word at flat offset {off} "
                             f"(payload starts at {buf.front}), {int(bad.sum())} words in all, value {int(iv[off]):#x}")


# ---------------------------------------------------------------------------------------------------------------------------
def elementwise_bound(terms_abs_sum, n_roundings):
    """n_roundings * 2**-24 * S_i (float64)"""
    return torch.as_tensor(terms_abs_sum, dtype=torch.float64) * (n_roundings * U)


def worst_ratio(got, want64, bound):
    """(ratio, flat index) of the element with the largest |got - want| / bound; bound 0 demands equality (ratio inf otherwise)"""
    got, want64, bound = got.detach().cpu().double().reshape(-1), want64.reshape(-1).double(), bound.reshape(-1).double()
    err = (got - want64).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    i = int(ratio.argmax())
    return float(ratio[i]), i


def assert_elementwise(got, want64, bound, what=""):
    """|got - want64| <= bound for every element; returns the worst ratio.  On failure: worst element's index, got, want, bound, ratio."""
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(want64)
    r, i = worst_ratio(got, want64, bound)
    if not r <= 1.0:
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), want64.shape))
        g, w, b = got.detach().cpu().double().reshape(-1)[i], want64.reshape(-1)[i], bound.reshape(-1)[i]
        raise AssertionError(f"{what}: element {idx}: got {float(g)!r}, want {float(w)!r}, bound {float(b):.3e}, ratio {r:.3g}")
    return r


# ---- transcendental-unit activations (csrc/common.h: ldc_silu / ldc_gelu_tanh = v * rcp(1 + exp2(t)), v_exp_f32 / v_rcp_f32) ----
# error of v * rcp(1 + 2^t) given the ABSOLUTE error dt of the exponent argument t (float64 tensors):
#   e = 2^t: relative ln2 * dt (argument) + 2 U (v_exp_f32, 1 ulp);  s = 1 + e: that times e / s, + U (the add);
#   rcp: 2 U (v_rcp_f32, 1 ulp);  v * r: U;  plus |v| TINY: a factor r under the smallest normal may be flushed to zero before the product
def _sigmoid_form_bound(v, t, dt):
    frac = torch.sigmoid(t * 0.6931471805599453)  # e / (1 + e) = sigmoid(ln 2^t), overflow-safe
    rel = frac * (0.6931471805599453 * dt + 2 * U) + U + 2 * U + U
    out = v * torch.sigmoid(-t * 0.6931471805599453)
    return out, out.abs() * rel + TINY * v.abs().clamp_min(1.0)


LOG2E = 1.4426950408889634


def silu_ref(v):
    """float64 (silu(v), rounding bound of ldc_silu at an exact input v): t = -log2(e) * v carries two roundings (the fp32 constant, the
    product), each |t| U absolute = |v| * log2(e) * 2**-24 in the exponent, i.e. |v| * log2(e) * 2**-24 * ln 2 relative in 2^t"""
    v = v.double()
    t = -LOG2E * v
    return _sigmoid_form_bound(v, t, 2 * U * t.abs())


GELU_C0 = -2.0 * 0.7978845608028654 * LOG2E
GELU_C1 = GELU_C0 * 0.044715


def gelu_tanh_ref(v):
    """float64 (gelu_tanh(v), bound of ldc_gelu_tanh): t = v * (c0 + c1 v v); c0: 1 rounding, c1 = c0 * 0.044715f: 3, c1 v v: +2, the sum:
    1 on each term, the product with v: 1 -> |dt| <= U (3 |c0 v| + 7 |c1 v^3|)"""
    v = v.double()
    t = v * (GELU_C0 + GELU_C1 * v * v)
    dt = U * (3 * (GELU_C0 * v).abs() + 7 * (GELU_C1 * v * v * v).abs())
    return _sigmoid_form_bound(v, t, dt)


ACT_MAX_SLOPE = {0: 1.0, 1: 1.1, 2: 1.13, 3: 1.0}  # max |act'|: identity, SiLU (1.0998), tanh-GELU (1.1289), ReLU


def act_ref(v64, bound_in, act):
    """float64 (act(v), bound) for the library's ldc_act codes, given the bound of the pre-activation: the input error passes through
    at most max |act'|, the activation's own roundings are added"""
    if act == 0:
        return v64, bound_in
    if act == 3:
        return v64.clamp_min(0), bound_in
    out, own = silu_ref(v64) if act == 1 else gelu_tanh_ref(v64)
    return out, ACT_MAX_SLOPE[act] * bound_in + own


# ---- operand-row formats (include/ladcast_hip.h: LDC_FMT_SPLIT / LDC_FMT_BF16) as bit images of fp32-typed buffers ----
FMT_F32, FMT_SPLIT, FMT_BF16 = 0, 1, 2


def operand_width(C, fmt):
    """payload width in FLOATS of a row of C values (C % 4 == 0; a last half group's pad half is written as zeros)"""
    cp = (C + 7) // 8 * 8
    return C if fmt == FMT_F32 else cp if fmt == FMT_SPLIT else cp // 2


def operand_rows(x, fmt):
    """fp32 [..., C] -> int32 bit image [..., operand_width(C, fmt)] of the row in format `fmt` (hi = bf16(x) RNE, lo = bf16(x - hi))"""
    x = x.float()
    C = x.shape[-1]
    if fmt == FMT_F32:
        return x.contiguous().view(torch.int32)
    cp = (C + 7) // 8 * 8
    xp = torch.nn.functional.pad(x, (0, cp - C))
    hi = xp.bfloat16()
    if fmt == FMT_BF16:
        return hi.contiguous().view(torch.int32)
    lo = (xp - hi.float()).bfloat16()
    lead = xp.shape[:-1]
    img = torch.stack([hi.reshape(*lead, cp // 8, 8), lo.reshape(*lead, cp // 8, 8)], dim=-2).reshape(*lead, 2 * cp)
    return img.contiguous().view(torch.int32)
