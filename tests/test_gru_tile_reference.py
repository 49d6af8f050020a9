"""The tile GRU model proven without a GPU.

tests/test_gpu_gru_tile.py holds gru_tile_fwd / gru_tile_bwd to three
limits: h_out within GRU_E32_FACTOR * e32 of the fp64 reference, bf16
outputs at most one ulp off on at most FLIP_CAP of the elements, dalpha
inside tests/gru_tile_reference.tile_bwd_ref's bound. This file shows that
an fp32 model of the kernels' arithmetic (operands split into bf16 terms,
two forward and three backward, fp32 accumulation, bf16 stores) meets each of them at every shape of
the table, so a kernel that misses one has a fault of its own, and that
the pieces of the model and of the bound are what they claim to be.
"""
import pytest
import torch

from tests import gru_tile_reference as TR
from tests import seq_reference as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
GRU_E32_FACTOR = 64.0       # tests/test_gpu_seq_kernels.py's, unchanged


def _ids(cases):
    return ["-".join(str(x) for x in (c if isinstance(c, tuple) else (c,)))
            .replace("(", "").replace(")", "").replace(", ", "x")
            for c in cases]


def test_split_residual():
    gen = torch.Generator().manual_seed(7)
    v = torch.randn(1 << 20, generator=gen) \
        * torch.pow(2.0, torch.randint(-20, 20, (1 << 20,), generator=gen))
    v = torch.cat([v, torch.tensor([1 + 2.0 ** -9 + 2.0 ** -17, 0.0, -0.0,
                                    1.0, 1 + 2.0 ** -8])])
    hi, lo, lo2 = TR.split(v, 3)
    # three terms are exact
    assert torch.equal(hi.double() + lo.double() + lo2.double(), v.double())
    # both terms are bf16 values and v - hi is exact in fp32
    assert torch.equal(hi, hi.to(BF16).float())
    assert torch.equal(lo, lo.to(BF16).float())
    assert torch.equal((v - hi).double(), v.double() - hi.double())
    res = (v.double() - hi.double() - lo.double()).abs()
    assert bool((res <= TR.SPLIT_WORST * v.double().abs()).all())
    tie = 1 + 2.0 ** -9 + 2.0 ** -17
    assert float(res[-5]) == 2.0 ** -17 and float(v[-5]) == tie
    # against a single rounding: 2**-8 |v|
    one = (v.double() - hi.double()).abs()
    assert bool((one <= R.BF * v.double().abs()).all())
    # the share of elements above the 2**-18 the bound terms use, and the
    # mean: a dot product's residual stays far inside 2**-18 |v| . |u|
    nz = v != 0
    rel = res[nz] / v.double().abs()[nz]
    print(f"split residual: max {float(rel.max()) * 2 ** 18:.3f} x 2^-18, "
          f"mean {float(rel.mean()) * 2 ** 18:.3f} x 2^-18, above 2^-18: "
          f"{float((rel > TR.SPLIT_REL).double().mean()):.4%}")
    assert float(rel.mean()) <= 0.5 * TR.SPLIT_REL


def test_tile_case_table():
    hs = [s[2] for s in TR.TILE_SHAPES]
    assert min(hs) == 1 and max(hs) == TR.MAX_H and 33 in hs and 36 in hs
    assert any(s[0] == 16 for s in TR.TILE_SHAPES)          # a full tile
    assert any(s[0] % 16 == 1 and s[0] > 16 for s in TR.TILE_SHAPES)
    assert any(s[0] % 16 == 15 for s in TR.TILE_SHAPES)
    assert any(s[0] > 64 for s in TR.TILE_SHAPES)           # a second block
    assert any(h % 16 == 0 for h in hs) and any(h % 16 for h in hs)
    assert any(h % 32 and h > 32 for h in hs)               # K padded to 64
    assert {s[2] for s in TR.E2E_SHAPES} == {36, 48, 63, 64}


@pytest.mark.parametrize("shape,augru", TR.TILE_ALL, ids=_ids(TR.TILE_ALL))
def test_model_forward_meets_the_gpu_limits(shape, augru):
    b, t, h = shape
    c = R.gru_case(b, t, h, augru)
    ref, gref = R.gru_fwd_ref(c["X3"], c["U"], c["bh"], c["alpha"])
    ref32, _ = R.gru_fwd_ref(c["X3"], c["U"], c["bh"], c["alpha"], dtype=F32)
    e32 = float((ref32.double() - ref).abs().max())
    got, gates = TR.tile_fwd_model(c["X3"], c["U"], c["bh"], c["alpha"])
    assert got.dtype == F32 and gates.dtype == BF16
    err = float((got.double() - ref).abs().max())
    assert e32 > 0
    print(f"tile model fwd {shape} augru={augru}: max err {err:.3e}, e32 "
          f"{e32:.3e}, ratio {err / e32:.2f}")
    assert err <= GRU_E32_FACTOR * e32
    n_ulp, share = R.ulp_flips(gates, gref)
    assert n_ulp <= 1 and share <= R.FLIP_CAP, (n_ulp, share)


@pytest.mark.parametrize("shape,augru", TR.TILE_ALL, ids=_ids(TR.TILE_ALL))
def test_model_backward_meets_the_gpu_limits(shape, augru):
    b, t, h = shape
    c = R.gru_case(b, t, h, augru)
    h64, g64 = R.gru_fwd_ref(c["X3"], c["U"], c["bh"], c["alpha"])
    h32, g16 = h64.float(), g64.float().to(BF16)
    dpx, dph, da, da_b = TR.tile_bwd_ref(c["dh_out"], h32, g16, c["U"],
                                         c["bh"], c["alpha"])
    # the reference inside tile_bwd_ref is seq_reference's, and the bound
    # is its bound plus non-negative terms
    sx, sh, sa, sa_b = R.gru_bwd_ref(c["dh_out"], h32, g16, c["U"], c["bh"],
                                     c["alpha"], with_bounds=True)
    assert torch.equal(dpx, sx) and torch.equal(dph, sh)
    got_x, got_h, got_a = TR.tile_bwd_model(c["dh_out"], h32, g16, c["U"],
                                            c["bh"], c["alpha"])
    what = f"tile model bwd {shape} augru={augru}"
    for name, got, ref in (("dpre_x", got_x, dpx), ("dpre_h", got_h, dph)):
        n_ulp, share = R.ulp_flips(got, ref)
        print(f"{what} {name}: {n_ulp:.2f} ulp, {share:.4%} differ")
        assert n_ulp <= 1 and share <= R.FLIP_CAP, (name, n_ulp, share)
    if augru:
        assert torch.equal(da, sa) and bool((da_b >= sa_b).all())
        if t > 1:
            assert bool((da_b[:, :-1] > sa_b[:, :-1]).any())
        R.assert_within(got_a, da, da_b, what + " dalpha")
        worst = float(((got_a.double() - da).abs()
                       / da_b.clamp(min=1e-300)).max())
        print(f"{what} dalpha: worst err / bound {worst:.3f}")
    else:
        assert got_a is None and da is None


def test_two_terms_miss_the_backward_ulp_rule():
    """Why the backward splits into three: with two, the model is several
    bf16 ulps off where dh_t or pn cancel."""
    worst = 0.0
    for shape in [(17, 7, 36), (15, 5, 48), (65, 4, 63)]:
        c = R.gru_case(*shape, True)
        h64, g64 = R.gru_fwd_ref(c["X3"], c["U"], c["bh"], c["alpha"])
        h32, g16 = h64.float(), g64.float().to(BF16)
        dpx, _, _ = R.gru_bwd_ref(c["dh_out"], h32, g16, c["U"], c["bh"],
                                  c["alpha"])
        got_x, _, _ = TR.tile_bwd_model(c["dh_out"], h32, g16, c["U"],
                                        c["bh"], c["alpha"], terms=2)
        worst = max(worst, R.ulp_flips(got_x, dpx)[0])
    assert worst > 1


def test_single_rounding_would_not_do():
    """What the split is for: h rounded once to bf16 misses the forward
    limit at the reference DIEN width."""
    b, t, h = 17, 7, 36
    c = R.gru_case(b, t, h, False)
    ref, _ = R.gru_fwd_ref(c["X3"], c["U"], c["bh"], None)
    ref32, _ = R.gru_fwd_ref(c["X3"], c["U"], c["bh"], None, dtype=F32)
    e32 = float((ref32.double() - ref).abs().max())
    x3, u_t, bias = c["X3"].float(), c["U"].float().t(), c["bh"]
    hv = torch.zeros(b, h)
    outs = []
    for i in range(t):
        hp = bias + hv.to(BF16).float() @ u_t
        xr, xz, xn = x3[:, i].split(h, 1)
        hr, hz, hn = hp.split(h, 1)
        r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
        n = torch.tanh(xn + r * hn)
        hv = (1 - z) * n + z * hv
        outs.append(hv)
    err = float((torch.stack(outs, 1).double() - ref).abs().max())
    assert err > GRU_E32_FACTOR * e32
