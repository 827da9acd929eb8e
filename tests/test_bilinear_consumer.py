"""Bilinear upsampling on activation codes: the contract, host logic and the CPU route (include/mctq_hip.h:
mctq_codes_upsample_bilinear_nhwc; hip/ops.py: codes_upsample_bilinear; consumers.QuantizedBilinearUpsample and the
``bilinear_upsamples`` switch of the rewrites).

The contract is on integers with 11-bit weights, so the reference is not reproduced bit for bit: the float64 interpolation of the
dequantized codes, coded in float64.  A code may differ from it by one, and only within ``tie_bound`` of a rounding tie."""
import numpy as np
import pytest
import torch

from test_upsample_consumer import IN_FORMS, OUT_FORMS, _form, _of, _targets, float_chain, holder_of, low_input, pot_conv

F = torch.nn.functional

# (arguments of F.interpolate, input H x W): the two dyadic factors, then align_corners, odd sizes, a fraction, down, one pixel
GEOMETRIES = [(dict(scale_factor=2), (9, 11)), (dict(scale_factor=4), (5, 3)), (dict(scale_factor=2, align_corners=True), (9, 11)),
              (dict(size=(13, 9)), (7, 5)), (dict(scale_factor=1.5), (9, 11)), (dict(size=(4, 5)), (9, 11)), (dict(scale_factor=3), (1, 1))]
# (input dtype, (scale, zero point)) -> output form: power-of-two scales with a zero point at the end of a type, and others
FORMS = {"pot": (torch.uint8, (1.0 / 32, 0), (1.0 / 16, -128, -128, 127)),
         "i8": (torch.int8, IN_FORMS["i8"][1:], OUT_FORMS["u8"]), "u8": (torch.uint8, IN_FORMS["u8"][1:], OUT_FORMS["i8"])}


def tables_of(geometry, h, w, device="cpu"):
    from mct_quantizers_amd import consumers
    q = holder_of("u4").activation_holder_quantizer
    return consumers.QuantizedBilinearUpsample(torch.nn.Upsample(mode="bilinear", **geometry), q, q).tables(h, w, device)


def random_codes(dtype, shape, seed=5):
    raw = torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed))
    return (raw - (128 if dtype == torch.int8 else 0)).to(dtype)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("index", range(len(GEOMETRIES)))
def test_the_contract_stays_within_one_code_of_float64_next_to_ties(index, form):
    from mct_quantizers_amd.hip import ops
    (geometry, (h, w)), (dtype, (s_a, z_a), out_form) = GEOMETRIES[index], FORMS[form]
    codes = random_codes(dtype, (2, h, w, 16), seed=index)
    got = ops.codes_upsample_bilinear(codes, (s_a, z_a), out_form, *tables_of(geometry, h, w))
    s_a, s_b = float(np.float32(s_a)), float(np.float32(out_form[0]))
    value = ((codes.double() - z_a) * s_a).permute(0, 3, 1, 2)
    r = F.interpolate(value, mode="bilinear", **geometry).permute(0, 2, 3, 1) / s_b          # in B's steps, float64
    want = (torch.round(r) + out_form[1]).clamp(out_form[2], out_form[3])
    # Each axis's weight is rounded to 11 bits, off by at most 2^-12: a value moves by at most 2 * 2^-12 * spread, the spread of
    # the four taps at most 255 codes of s_a.  The float32 route rounds four times (the conversion of acc, the product with
    # s_a * 2^-22, the reciprocal 1 / s_b, the product with it), each by at most 2^-24 relative, on |r| <= 255 * s_a / s_b; a
    # fifth 2^-24 covers their second-order terms and the float64 roundings of the reference and of the ramps (2^-52 each).
    tie_bound = (2.0 ** -11 + 5 * 2.0 ** -24) * 255 * s_a / s_b
    differs = got.double() != want
    print(f"{geometry} {form}: {differs.double().mean():.4f} differ, tie bound {tie_bound:.4f}")
    assert (got.double() - want).abs().max() <= 1
    assert bool((((r - r.floor()) - 0.5).abs()[differs] <= tie_bound).all())
    if index < 2 and form == "pot":                          # dyadic weights, power-of-two scales: the float32 chain bit for bit
        assert not differs.any() and torch.equal(got, float_chain(codes, (s_a, z_a), out_form, dict(mode="bilinear", **geometry)))
        assert got.dtype == torch.int8 and len(torch.unique(got)) > 50


def test_other_channel_counts_empty_shapes_and_clamped_tables():
    from mct_quantizers_amd.hip import ops
    rows, cols = tables_of(dict(scale_factor=2), 3, 4)
    x, a, out = random_codes(torch.uint8, (2, 3, 4, 21)), (0.1, 3), (0.05, -3, -128, 127)
    whole = ops.codes_upsample_bilinear(x, a, out, rows, cols)
    assert torch.equal(whole[..., :16], ops.codes_upsample_bilinear(x[..., :16], a, out, rows, cols))
    assert ops.codes_upsample_bilinear(x[:0], a, out, rows, cols).shape == (0, 6, 8, 21)
    wild = ((rows[0] - 9, rows[1] + 9, rows[2] * 5 - 4000), (cols[0] + 7, cols[1] - 7, cols[2]))
    tame = ((rows[0] * 0, rows[1] * 0 + 2, (rows[2] * 5 - 4000).clamp(0, 2048)), (cols[0] * 0 + 3, cols[1] * 0, cols[2]))
    assert torch.equal(ops.codes_upsample_bilinear(x, a, out, *wild), ops.codes_upsample_bilinear(x, a, out, *tame))
    with pytest.raises(ValueError, match="one length"):
        ops.codes_upsample_bilinear(x, a, out, rows, (cols[0], cols[1], cols[2][:3]))


class Head(torch.nn.Module):
    """conv -> A -> bilinear 2x -> B -> conv1x1, power-of-two forms throughout: every product and blend is exact in float32."""

    def __init__(self, how):
        super().__init__()
        self.how = how
        self.h0, self.first, self.ha = holder_of("s4"), pot_conv(16, 16, 3, 1), holder_of("u4")
        self.up = torch.nn.UpsamplingBilinear2d(scale_factor=2) if how == "2d" else torch.nn.Upsample(scale_factor=2, mode="bilinear")
        self.hb, self.last = holder_of("u8"), pot_conv(16, 32, 1, 2)

    def forward(self, x):
        a = self.ha(self.first(self.h0(x)))
        if self.how == "functional":
            u = F.interpolate(a, scale_factor=2.0, mode="bilinear", align_corners=False)
        elif self.how == "dynamic":
            u = F.interpolate(a, size=(x.shape[2] * 2, x.shape[3] * 2), mode="bilinear")
        elif self.how == "antialias":
            u = F.interpolate(a, scale_factor=2.0, mode="bilinear", antialias=True)
        else:
            u = self.up(a)
        return self.last(self.hb(u))


@pytest.mark.parametrize("how", ["module", "2d", "functional", "dynamic", "antialias"])
def test_the_rewrite_takes_a_bilinear_upsample_between_two_holders(how, device="cpu"):
    from mct_quantizers_amd import consumers as C
    x = low_input(device)
    with torch.no_grad():
        want = Head(how).to(device)(x)
    for switches in (dict(), dict(convolutions=True, shared_holders=True, stay_on_codes=True, pools=True, concats=True)):
        gm, n = C.fuse_linear_consumers_fx(Head(how).to(device), bilinear_upsamples=True, **switches)
        gm0, n0 = C.fuse_linear_consumers_fx(Head(how).to(device), **switches)
        gm1, n1 = C.fuse_linear_consumers_fx(Head(how).to(device), upsamples=True, **switches)
        assert n0 == n1 and str(gm0.graph) == str(gm1.graph) and gm0.code == gm1.code and not _of(gm0, C.QuantizedBilinearUpsample)
        if how in ("dynamic", "antialias"):                  # left alone: the graph is the one without the switch
            assert n == n0 and str(gm.graph) == str(gm0.graph) and gm.code == gm0.code
            continue
        assert list(_of(gm, C.QuantizedBilinearUpsample)) == ["hb_bilinear"] and "hb" not in _targets(gm) and n == n0
        q = gm.get_submodule("hb_bilinear")
        assert q.activation_code_params() == _form(Head(how).ha) and q.output_code_params() == _form(Head(how).hb)
        seen = []
        hook = q.register_forward_hook(lambda m, args, out: seen.append((args[0], out)))
        y = gm(x)
        hook.remove()
        module = C.QuantizedBilinearUpsample(q.upsample, q.in_quantizer, q.out_quantizer)
        assert torch.equal(module(seen[0][0].cpu()), seen[0][1].cpu())                   # the module route, on the CPU
        if how != "2d":                                      # dyadic weights: the model as built, bit for bit
            assert torch.equal(y, want) and torch.equal(y, gm0(x))
        assert y.shape == (2, 32, 8, 10) and len(torch.unique(y)) > 50
    seq = torch.nn.Sequential(holder_of("u4"), torch.nn.Upsample(scale_factor=2, mode="bilinear"), holder_of("u8"), pot_conv(16, 32, 1, 2))
    assert C.fuse_linear_consumers(seq, bilinear_upsamples=True) == 1 and type(seq[1]) is C.QuantizedBilinearUpsample
    assert C.QuantizedBilinearUpsample in C._CODE_READERS and not C.QuantizedUpsample.eligible(seq[1].upsample)


def test_the_entry_point_refuses_bad_arguments_without_a_launch(P=4096):
    from mct_quantizers_amd.hip import native
    lib = native.load()
    count = lib.mctq_launch_count()
    T = P + 8192                                              # the tables' address; out at P (2 * 4 * 4 * 16 bytes), the codes behind

    def call(codes=P + 4096, out=P, dt=native.CODE_U8, in_zp=3, in_scale=0.1, b=2, h=2, w=2, c=16, ho=4, wo=4, tables=(T,) * 6,
             odt=native.CODE_I8, scale=0.05, zp=-3, qmin=-128, qmax=127):
        rc = lib.mctq_codes_upsample_bilinear_nhwc(codes, out, dt, in_zp, in_scale, b, h, w, c, ho, wo, *tables, odt, scale, zp, qmin, qmax, None)
        return rc, lib.mctq_last_error()

    for message, fault in ((b"negative extent", dict(ho=-1)), (b"channels must be a multiple of 16", dict(c=24)),
                           (b"bad code_dtype", dict(dt=7)), (b"in_zero_point is no code of the input's type", dict(in_zp=256)),
                           (b"scale must be finite and positive", dict(scale=float("inf"))), (b"quant_min > quant_max", dict(qmin=9, qmax=8)),
                           (b"a non-empty output needs an image of at least one pixel", dict(h=0)),
                           (b"more than 2^31 - 1 16-byte chunks of output in one launch", dict(b=2 ** 20, ho=2 ** 10, wo=2 ** 10)),
                           (b"NULL pointer", dict(out=None)), (b"NULL table", dict(tables=(T, T, None, T, T, T))),
                           (b"codes and out must be 16-byte aligned", dict(codes=P + 4100)),
                           (b"the tables must be 4-byte aligned", dict(tables=(T,) * 5 + (T + 2,))),
                           (b"out overlaps codes", dict(codes=P + 496)), (b"out overlaps a table", dict(tables=(T,) * 4 + (P - 12, T)))):
        assert call(**fault) == (native.MCTQ_E_ARG, message), fault
    assert call(b=0, codes=None, out=None)[0] == 0 and call(ho=0, tables=(None,) * 6)[0] == 0      # empty: before any pointer check
    assert lib.mctq_set_tuning(b"bilinear_strip", 2) == native.MCTQ_E_ARG and lib.mctq_set_tuning(b"bilinear_strip", 0) == 0
    assert lib.mctq_launch_count() == count
