"""Exact-integer references for the MFMA linear kernels (CPU only).

The operands are integer-valued bf16 matrices, so every product and every
partial sum of fwd / dX / dW is an integer far below 2**24: fp32 MFMA
accumulation and fp32 atomicAdd are exact and order-independent, and an
int64 matmul on the CPU is the bit-exact reference. The only rounding left
is the kernel's final fp32 -> bf16 store, which must agree with torch's
round-to-nearest-even.

tests/test_dense_reference.py proves the preconditions (magnitudes, bf16
round-trips, share of outputs that really round) for every shape below
without a GPU; tests/test_gpu_dense_shapes.py runs the kernels on them.

Layouts: x[M,K], w[N,K], g[M,N].
"""
import functools

import torch

# (M, N, K) — the smallest shapes that reach each kernel path
FWD_SHAPES = [
    (16, 1, 64),      # N = 1 (every tower's last layer)
    (80, 72, 45),     # full 64-col tile next to a partial one, K tail
                      # crossing an 8-wide fragment
    (80, 72, 429),    # odd K of the zoo's first layer (13 + 26*16)
    (100, 100, 16),   # M % 16 != 0, N % 8 != 0
    (130, 64, 8),     # 2 rows in the last block, K < 32; MT=2: 2nd block
    (340, 96, 20),    # GRU projection: M = 17*20, N = 3H
]
DX_SHAPES = [
    (100, 1, 45),     # direct kernel, GEMM-K = 1
    (80, 127, 72),    # direct kernel, just below the N >= 128 dispatch
    (80, 128, 64),    # LDS kernel, at the threshold
    (130, 300, 45),   # LDS: superchunk + 44-row remainder, idle waves
    (16, 1024, 429),  # LDS kernel at the zoo's shape
    (340, 96, 20),    # direct kernel, GRU shape
]
DW_SHAPES = [
    (130, 1, 45),       # N = 1
    (130, 72, 45),      # two M chunks, the second one 2 rows
    (1000, 100, 429),   # ragged M and N, odd K
    (340, 96, 32),      # GRU shape
    (4934, 200, 429),   # variant 2: 39 chunks, cpb = 2, last block 1 chunk
]
# linear_dw_out into a flat-buffer slice: N*K + N is no multiple of 4, so
# the zero-fill has a scalar tail; N = 1 and N >= 64 take different kernels.
# The last workspace is shorter than one float4: head and tail only.
DW_OUT_SHAPES = [(130, 1, 45), (130, 75, 45), (16, 1, 2)]

# at K = 429 this spreads the sums past 256 often enough that >= 5 % of
# the outputs are not bf16-representable
FWD_RANGE = (-4, 4)
DW_RANGE = (-3, 3)
# dX sums only N products: the wider range pushes most results past 256,
# where odd integers are no longer bf16-representable and must round
DX_RANGE = (-7, 7)

EXACT_LIMIT = 2 ** 24     # integers below this are exact in fp32
SIGMOID_LIMIT = 8.0       # |pre-activation| bound for the act = 2 cases
GUARD = 64                # NaN elements in front of and behind an operand


def int_matrix(rows, cols, rng, seed):
    """Random per-element integers in [rng[0], rng[1]] as int64."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(rng[0], rng[1] + 1, (rows, cols), generator=gen,
                         dtype=torch.int64)


def half_bias(n, seed):
    """fp32 bias, multiples of 0.5 in [-2, 2]."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, (n,), generator=gen).float() * 0.5


def bf16_exact(t):
    """True if every element of t survives a bf16 round-trip unchanged."""
    return torch.equal(t.to(torch.bfloat16).to(t.dtype), t)


def to_bf16_rne(exact):
    """Round exact fp64 values to bf16. They are exactly representable in
    fp32 (asserted), so fp64 -> fp32 -> bf16 rounds once, to nearest even."""
    f32 = exact.float()
    assert torch.equal(f32.double(), exact), "value not exact in fp32"
    return f32.to(torch.bfloat16)


def inexact_fraction(exact):
    """Share of the values that are not bf16-representable."""
    return (to_bf16_rne(exact).double() != exact).double().mean().item()


def tie_count(exact):
    """Number of values exactly half-way between two bf16 neighbours."""
    f32 = exact.float()
    bits = f32.view(torch.int32)
    return int(((bits & 0xFFFF) == 0x8000).sum())


def apply_act(pre, act):
    if act == 1:
        return torch.relu(pre)
    if act == 2:
        return torch.sigmoid(pre)
    return pre


@functools.lru_cache(maxsize=None)
def fwd_case(m, n, k):
    """x, w as int64; bias fp32; pre = x @ w^T (+ bias) exact in fp64."""
    seed = 1000003 * m + 1009 * n + k
    x = int_matrix(m, k, FWD_RANGE, seed)
    w = int_matrix(n, k, FWD_RANGE, seed + 1)
    bias = half_bias(n, seed + 2)
    ref = x @ w.t()
    return {"x": x, "w": w, "bias": bias, "ref": ref,
            "pre_bias": ref.double() + bias.double(),
            "pre_nobias": ref.double()}


def sigmoid_shift(ref_int, bias):
    """Smallest s with max|ref| * 2**-s + max|bias| <= SIGMOID_LIMIT. The
    act = 2 cases scale w by 2**-s — still exact in bf16 and fp32."""
    peak = float(ref_int.abs().max())
    room = SIGMOID_LIMIT - float(bias.abs().max())
    s = 0
    while peak * 2.0 ** -s > room:
        s += 1
    return s


@functools.lru_cache(maxsize=None)
def dx_case(m, n, k):
    seed = 2000003 * m + 2003 * n + k
    g = int_matrix(m, n, DX_RANGE, seed)
    w = int_matrix(n, k, DX_RANGE, seed + 1)
    return {"g": g, "w": w, "ref": g @ w}


@functools.lru_cache(maxsize=None)
def dw_case(m, n, k):
    seed = 3000017 * m + 3001 * n + k
    g = int_matrix(m, n, DW_RANGE, seed)
    x = int_matrix(m, k, DW_RANGE, seed + 1)
    return {"g": g, "x": x, "dw": g.t() @ x, "db": g.sum(0)}


def dw_cpb(m, n, k):
    """(m_chunks, cpb) of the variant-2 dW launch — the formula of
    linear_dw_impl in ops/hip/dense_kernels.hip."""
    m_chunks = (m + 127) // 128
    tiles = ((n + 63) // 64) * ((k + 63) // 64)
    return m_chunks, max(1, m_chunks * tiles // 512)


def carve(values, device, offset=GUARD, tail=GUARD, fill=float("nan")):
    """Copy `values` into a larger flat buffer on `device` whose remainder
    is `fill`, and return (contiguous view shaped like values, flat buffer,
    offset). A kernel that reads past the operand and uses what it finds
    turns an integer result into NaN."""
    flat = torch.full((offset + values.numel() + tail,), fill,
                      dtype=values.dtype, device=device)
    view = flat[offset:offset + values.numel()].view(values.shape)
    view.copy_(values)
    return view, flat, offset


def outside_untouched(flat, offset, numel, fill):
    """True if every element of flat outside [offset, offset+numel) still
    holds `fill` (NaN compares by isnan)."""
    rest = torch.cat([flat[:offset], flat[offset + numel:]])
    if fill != fill:
        return bool(torch.isnan(rest).all())
    return bool((rest == fill).all())


def linear_bounds(a, b, ref, red):
    """Per-element error bound of a bf16-output MFMA GEMM with fp32
    accumulation over `red` terms: one bf16 rounding of the result plus
    fp32 accumulation, 2**-8 |ref| + red * 2**-23 * (|a| @ |b|)."""
    acc = red * 2.0 ** -23 * (a.abs() @ b.abs())
    return 2.0 ** -8 * ref.abs() + acc, acc
