"""Nearest upsampling on activation codes: host logic and the CPU route (include/mctq_hip.h: mctq_codes_upsample_nhwc;
hip/ops.py: codes_upsample; consumers.QuantizedUpsample and the ``upsamples`` switch of the rewrites).

Everything here is exact, so every check is equality.  A holder's float32 output is ``float(code - zp) * scale`` bit for bit and
nearest interpolation only moves data, so the codes the holder behind an upsample gives are the input's codes gathered through
the upsample's index map and requantized one by one.  The op is pinned against that definition written in numpy float32 and
against the literal float32 chain around ``F.interpolate``.

A model rewritten with ``upsamples=True`` is compared bit for bit with the same rewrite without it and with the model as built;
the models are built as those of tests/test_concat_consumer.py are (power-of-two scales, no bias, short sums: exact products)."""
import functools

import numpy as np
import pytest
import torch

from test_concat_consumer import _form, holder_of
from test_join_consumer import _targets
from test_pool_consumer import _of, pot_conv

F = torch.nn.functional

# ---- the op's cases: shared by the CPU and GPU tests --------------------------------------------------------------------------

# the arguments of nn.Upsample / F.interpolate: integer factors, fractional ones, downsampling, a recomputed factor, sizes
GEOMETRIES = [dict(scale_factor=2), dict(scale_factor=(1.5, 2.7)), dict(scale_factor=(3, 1)), dict(scale_factor=0.5),
              dict(scale_factor=2.5, recompute_scale_factor=True), dict(size=(7, 5)),
              dict(size=(13, 29), mode="nearest-exact"), dict(scale_factor=1.3, mode="nearest-exact")]
# the integer factors of a 9 x 11 input among them, None elsewhere
FACTORS = [(2, 2), None, (3, 1), None, None, None, None, None]
IN_SHAPE = (2, 9, 11)                                        # batch, height, width

# (int8?, scale, zero point) of the input; (scale, zero point, qmin, qmax) of the output: no scale is a power of two
IN_FORMS = {"u8": (False, 0.061, 114), "i8": (True, 0.05, -5)}
OUT_FORMS = {"u8": (0.025, 114, 0, 255), "i8": (0.03, -5, -128, 127), "u4": (0.37, 3, 0, 15), "i7": (0.04, 9, -64, 63)}


def upsample_reference(codes, in_form, out_form, rows, cols):
    """The definition in numpy float32: codes [B, H, W, C] -> [B, Ho, Wo, C] through the maps ``rows`` [Ho], ``cols`` [Wo]."""
    (s_in, z_in), (scale, zp, qmin, qmax) = in_form, out_form
    f32 = np.float32
    moved = codes[:, np.asarray(rows)][:, :, np.asarray(cols)]
    v = (moved.astype(np.int32) - np.int32(z_in)).astype(f32) * f32(s_in)           # the holder's float32 output, resampled
    q = np.rint(v * (f32(1.0) / f32(scale))).astype(f32) + f32(zp)
    return np.clip(q, f32(qmin), f32(qmax)).astype(np.int32).astype(np.uint8 if qmin >= 0 else np.int8)


def float_chain(codes, in_form, out_form, geometry):
    """The literal chain in torch float32 on the codes' device: dequantize, ``F.interpolate``, ``fq_codes`` in the output form."""
    from mct_quantizers_amd.hip import ops
    value = ops.dequantize_codes(codes, *in_form).permute(0, 3, 1, 2)               # NCHW-shaped, NHWC-stored
    up = F.interpolate(value, **geometry)
    scale, zp, qmin, qmax = out_form
    return ops.fq_codes(up, None, None, None, qmin, qmax, scale, zp).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def index_maps(index, height=IN_SHAPE[1], width=IN_SHAPE[2]):
    """(src_rows, src_cols) of GEOMETRIES[index] as int64 CPU tensors, read off ``F.interpolate`` of two coordinate ramps -- not
    the module's derivation, which is checked against this one."""
    ys = torch.arange(height, dtype=torch.float32).reshape(1, 1, height, 1).expand(1, 1, height, width)
    xs = torch.arange(width, dtype=torch.float32).reshape(1, 1, 1, width).expand(1, 1, height, width)
    rows, cols = F.interpolate(ys, **GEOMETRIES[index])[0, 0], F.interpolate(xs, **GEOMETRIES[index])[0, 0]
    assert bool((rows == rows[:, :1]).all()) and bool((cols == cols[:1]).all())      # separable
    return rows[:, 0].to(torch.int64), cols[0].to(torch.int64)


@functools.lru_cache(maxsize=None)
def upsample_case(index, channels, in_kind="u8", out_kind="i8"):
    """(codes, in_form, out_form, the reference's result) for GEOMETRIES[index] on a 2 x 9 x 11 x channels input, computed once
    and shared; read-only."""
    signed, s, z = IN_FORMS[in_kind]
    rng = np.random.default_rng(100 * index + channels)
    shape = IN_SHAPE + (channels,)
    codes = rng.integers(-128, 128, shape).astype(np.int8) if signed else rng.integers(0, 256, shape).astype(np.uint8)
    rows, cols = index_maps(index)
    want = upsample_reference(codes, (s, z), OUT_FORMS[out_kind], rows.numpy(), cols.numpy())
    codes.setflags(write=False)
    want.setflags(write=False)
    return codes, (s, z), OUT_FORMS[out_kind], want


def all_codes(signed):
    """Every code of the type once, as [1, 4, 4, 16] codes (one 16-byte chunk per pixel)."""
    return (np.arange(-128, 128).astype(np.int8) if signed else np.arange(256).astype(np.uint8)).reshape(1, 4, 4, 16)


# (input kind, output form): the four type pairs, a clamp narrower than the type, and the pairs whose two forms are identical
EVERY_CODE_PAIRS = [("u8", OUT_FORMS["u8"]), ("u8", OUT_FORMS["i8"]), ("i8", OUT_FORMS["u8"]), ("i8", OUT_FORMS["i8"]),
                    ("u8", OUT_FORMS["u4"]), ("i8", OUT_FORMS["i7"]), ("u8", (0.061, 114, 0, 255)), ("i8", (0.05, -5, -128, 127))]


def t(array, device="cpu"):
    return torch.from_numpy(np.array(array)).to(device)


def test_the_cases_cover_what_they_should():
    assert len(GEOMETRIES) == 8 and [g for g, f in zip(GEOMETRIES, FACTORS) if f] == [dict(scale_factor=2), dict(scale_factor=(3, 1))]
    sizes = [(len(index_maps(i)[0]), len(index_maps(i)[1])) for i in range(8)]
    assert sizes == [(18, 22), (13, 29), (27, 11), (4, 5), (22, 27), (7, 5), (13, 29), (11, 14)]
    # nearest and nearest-exact differ on the same output size
    assert not torch.equal(index_maps(1)[0], index_maps(6)[0])
    for kind, out_form in EVERY_CODE_PAIRS[:6]:
        want = upsample_reference(all_codes(kind == "i8"), IN_FORMS[kind][1:], out_form, [0, 1, 2, 3], [0, 1, 2, 3])
        assert want.min() == out_form[2] and want.max() == out_form[3]                   # both ends of the clamp are reached


# ---- the op ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("index", range(len(GEOMETRIES)))
def test_codes_upsample_on_cpu_equals_the_reference_and_the_float_chain(index):
    from mct_quantizers_amd.hip import ops
    rows, cols = index_maps(index)
    for channels in (16, 48, 5):
        for in_kind, out_kind in (("u8", "i8"), ("i8", "u8")):
            codes, in_form, out_form, want = upsample_case(index, channels, in_kind, out_kind)
            got = ops.codes_upsample(t(codes), in_form, out_form, rows, cols)
            assert got.dtype == (torch.uint8 if out_form[2] >= 0 else torch.int8) and got.is_contiguous()
            assert tuple(got.shape) == want.shape and np.array_equal(got.numpy(), want), (index, channels)
            assert torch.equal(got, float_chain(t(codes), in_form, out_form, GEOMETRIES[index])), (index, channels)
            assert torch.equal(got, ops.codes_upsample(t(codes), in_form, out_form, rows.to(torch.int32), cols.to(torch.int32)))
            if FACTORS[index]:
                assert torch.equal(got, ops.codes_upsample(t(codes), in_form, out_form, rows, cols, factors=FACTORS[index]))


def test_every_code_for_every_type_pair_on_cpu():
    from mct_quantizers_amd.hip import ops
    rows = cols = torch.arange(8) // 2
    for kind, out_form in EVERY_CODE_PAIRS:
        codes = all_codes(kind == "i8")
        in_form = IN_FORMS[kind][1:]
        got = ops.codes_upsample(t(codes), in_form, out_form, rows, cols)
        assert np.array_equal(got.numpy(), upsample_reference(codes, in_form, out_form, rows.numpy(), cols.numpy())), (kind, out_form)
        assert torch.equal(got, float_chain(t(codes), in_form, out_form, dict(scale_factor=2)))
        if in_form == out_form[:2]:                                                     # the copy case: the codes come back
            assert torch.equal(got, t(codes)[:, rows][:, :, cols])


def test_codes_upsample_validation_and_edges():
    from mct_quantizers_amd.hip import ops
    u8 = torch.zeros(2, 3, 4, 16, dtype=torch.uint8)
    rows, cols = torch.arange(6) // 2, torch.arange(8) // 2
    out = (0.1, 0, 0, 255)
    with pytest.raises(ValueError, match="N, H, W, C"):
        ops.codes_upsample(u8[0], (0.1, 0), out, rows, cols)
    with pytest.raises(NotImplementedError):
        ops.codes_upsample(u8.float(), (0.1, 0), out, rows, cols)
    with pytest.raises(ValueError, match="zero point"):
        ops.codes_upsample(u8, (0.1, -1), out, rows, cols)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scales"):
            ops.codes_upsample(u8, (bad, 0), out, rows, cols)
        with pytest.raises(ValueError, match="scales"):
            ops.codes_upsample(u8, (0.1, 0), (bad, 0, 0, 255), rows, cols)
    with pytest.raises(ValueError, match="8-bit code"):
        ops.codes_upsample(u8, (0.1, 0), (0.1, 0, -1, 255), rows, cols)
    with pytest.raises(TypeError, match="src_rows"):
        ops.codes_upsample(u8, (0.1, 0), out, rows.float(), cols)
    with pytest.raises(TypeError, match="src_cols"):
        ops.codes_upsample(u8, (0.1, 0), out, rows, cols.reshape(2, 4))
    with pytest.raises(ValueError, match="at least one pixel"):
        ops.codes_upsample(u8[:, :0], (0.1, 0), out, rows, cols)
    # entries outside the image are clamped into it, as the kernel clamps them
    x = torch.randint(0, 256, (2, 3, 4, 16), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    assert torch.equal(ops.codes_upsample(x, (0.1, 0), out, rows + 2, cols - 1),
                       ops.codes_upsample(x, (0.1, 0), out, (rows + 2).clamp(0, 2), (cols - 1).clamp(0, 3)))
    # an empty batch, no channels, an empty map; a non-contiguous input
    assert ops.codes_upsample(u8[:0], (0.1, 0), out, rows, cols).shape == (0, 6, 8, 16)
    assert ops.codes_upsample(u8[..., :0], (0.1, 0), (0.1, 0, -128, 127), rows, cols).dtype == torch.int8
    assert ops.codes_upsample(u8, (0.1, 0), out, rows[:0], cols).shape == (2, 0, 8, 16)
    x = torch.randint(0, 256, (3, 2, 4, 16), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    assert torch.equal(ops.codes_upsample(x.permute(1, 0, 2, 3), (0.1, 0), out, rows, cols),
                       ops.codes_upsample(x.permute(1, 0, 2, 3).contiguous(), (0.1, 0), out, rows, cols))
    # the helper that turns host-side maps into factors
    assert ops.integer_factor(torch.arange(12) // 3, 4) == 3 and ops.integer_factor([0, 1, 2], 3) == 1
    assert ops.integer_factor(torch.arange(12) // 4, 4) is None and ops.integer_factor([0, 0, 1, 2], 2) is None
    assert ops.integer_factor([0, 1], 3) is None and ops.integer_factor([], 3) is None and ops.integer_factor([0], 0) is None


# ---- the module ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("index", range(len(GEOMETRIES)))
def test_the_module_reads_the_maps_interpolate_itself_uses(index):
    from mct_quantizers_amd import consumers
    geometry = GEOMETRIES[index]
    q = consumers.QuantizedUpsample(torch.nn.Upsample(**geometry), holder_of("s").activation_holder_quantizer)
    rows, cols, factors = q.index_maps(9, 11, "cpu")
    assert rows.dtype == cols.dtype == torch.int32 and factors == FACTORS[index]
    want_rows, want_cols = index_maps(index)
    assert torch.equal(rows.long(), want_rows) and torch.equal(cols.long(), want_cols)
    x = torch.randn(2, 3, 9, 11, generator=torch.Generator().manual_seed(index))
    for xx in (x, x.contiguous(memory_format=torch.channels_last)):
        y = F.interpolate(xx, **geometry)
        assert torch.equal(y, xx[:, :, rows.long()][:, :, :, cols.long()])
    assert y.is_contiguous(memory_format=torch.channels_last)                           # channels-last in, channels-last out
    assert q.index_maps(9, 11, torch.device("cpu")) is q.index_maps(9, 11, "cpu")          # cached
    # another input shape has maps of its own; a shape beyond 2^24 pixels takes the two-ramp form, here forced on a small one
    rows2, cols2, _ = q.index_maps(5, 4, "cpu")
    z = torch.randn(1, 1, 5, 4)
    assert torch.equal(F.interpolate(z, **geometry), z[:, :, rows2.long()][:, :, :, cols2.long()])


def test_the_two_ramp_form_gives_the_same_maps(monkeypatch):
    from mct_quantizers_amd import consumers
    q = consumers.QuantizedUpsample(torch.nn.Upsample(scale_factor=(1.5, 2.7)), holder_of("s").activation_holder_quantizer)
    one = q.index_maps(9, 11, "cpu")
    q2 = consumers.QuantizedUpsample(torch.nn.Upsample(scale_factor=(1.5, 2.7)), holder_of("s").activation_holder_quantizer)
    monkeypatch.setattr(consumers, "_ONE_RAMP_MAX", 10)
    two = q2.index_maps(9, 11, "cpu")
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]) and one[2] == two[2]


def test_eligible():
    from mct_quantizers_amd import consumers
    E, U = consumers.QuantizedUpsample.eligible, torch.nn.Upsample
    for geometry in GEOMETRIES:
        assert E(U(**geometry))
    assert E(torch.nn.UpsamplingNearest2d(scale_factor=2)) and E(torch.nn.UpsamplingNearest2d(size=(8, 10))) and E(U(size=7))
    assert E(U(scale_factor=2.0, recompute_scale_factor=False)) and E(U(size=[8, 10]))
    for bad in (U(scale_factor=2, mode="bilinear"), U(scale_factor=2, mode="bicubic"), U(scale_factor=2, mode="area"),
                U(scale_factor=2, mode="bilinear", align_corners=True), U(scale_factor=2, mode="nearest", align_corners=True),
                U(scale_factor=(2,)), U(scale_factor=(2, 2, 2)), U(size=(4,)), U(size=(4, 4, 4)), U(scale_factor=2, mode="linear"),
                U(scale_factor=2, mode="trilinear"), U(), U(size=(4.5, 4)), U(scale_factor=(-1.0, 2.0)), U(size=(0, 4)),
                torch.nn.UpsamplingBilinear2d(scale_factor=2), torch.nn.PixelShuffle(2), torch.nn.ConvTranspose2d(16, 16, 2, 2),
                torch.nn.Identity(), None, "nearest"):
        assert not E(bad), bad
    both = U(scale_factor=2)
    both.size = (4, 4)
    assert not E(both)
    with pytest.raises(TypeError):
        consumers.QuantizedUpsample(U(scale_factor=2, mode="bilinear"), holder_of("s").activation_holder_quantizer)


def check_upsample_module(device):
    """QuantizedUpsample on float32 and on codes, nearest and nearest-exact, integer and other geometry, with and without a
    holder behind, against the holders around the upsample on the CPU; returns the outputs."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    outs = []
    for geometry, kinds, channels in ((GEOMETRIES[0], ("s", "uni"), 16), (GEOMETRIES[1], ("uni", "u4"), 32), (GEOMETRIES[6], ("u4", "s"), 16),
                                      (GEOMETRIES[3], ("s", None), 16), (GEOMETRIES[7], ("u8", "s4"), 24)):
        up, ha, hb = torch.nn.Upsample(**geometry), holder_of(kinds[0]), holder_of(kinds[1]) if kinds[1] else None
        q = consumers.QuantizedUpsample(up, ha.activation_holder_quantizer, hb.activation_holder_quantizer if hb else None)
        assert q.activation_code_params() == _form(ha) and q.output_code_params() == _form(hb or ha)
        s, z, qmin, qmax = q.output_code_params()
        x = (torch.randn(2, channels, 9, 11, generator=torch.Generator().manual_seed(31)) * 3.0).to(device)
        with torch.no_grad():
            want = up(ha(x.cpu()))
            want = hb(want) if hb else want
        y = q(x)
        assert y.dtype == ops._code_dtype(qmin, qmax)[0] and y.shape == want.shape
        assert y.is_contiguous(memory_format=torch.channels_last)                       # NCHW-shaped, NHWC-stored
        assert torch.equal(ops.dequantize_codes(y.cpu(), s, z), want) and len(torch.unique(y)) > 20
        a = _form(ha)
        codes = ops.fq_codes_nhwc(x, a[2], a[3], a[0], a[1]).permute(0, 3, 1, 2)
        assert torch.equal(q(codes), y)                                                 # codes in
        assert torch.equal(q(x.contiguous(memory_format=torch.channels_last)), y)
        with torch.no_grad():
            assert torch.equal(q(ha(x.cpu()).to(device)), y)                            # the holder's output: the same codes
        wrong = torch.int8 if codes.dtype == torch.uint8 else torch.uint8
        with pytest.raises(TypeError):
            q(codes.to(wrong))
        with pytest.raises(TypeError):
            q(x.double())
        with pytest.raises(RuntimeError):
            q(x[0])
        outs.append(y.cpu())
    return outs


def test_quantized_upsample_on_cpu():
    import warnings
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    assert len(check_upsample_module("cpu")) == 5
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wide = mq.pytorch_quantizers.ActivationSymmetricInferableQuantizer(num_bits=16, threshold=[4.0], signed=True)
    ok, up = holder_of("u4").activation_holder_quantizer, torch.nn.Upsample(scale_factor=2)
    with pytest.raises(NotImplementedError):
        consumers.QuantizedUpsample(up, wide, ok)
    with pytest.raises(NotImplementedError):
        consumers.QuantizedUpsample(up, ok, wide)
    assert consumers.QuantizedUpsample in consumers._CODE_READERS


# ---- the rewrite -----------------------------------------------------------------------------------------------------------

class Chain(torch.nn.Module):
    """conv -> ReLU -> A -> Upsample(2x) -> [B ->] conv1x1 (``second``: with B; ``how``: the upsample as a module or as a call of
    ``F.interpolate``; ``two``: two convolutions behind, one of them behind a max pool)."""

    def __init__(self, second=True, how="module", two=False):
        super().__init__()
        self.how, self.two = how, two
        self.h0 = holder_of("s4")
        self.first = pot_conv(16, 16, 3, 1)
        self.ha = holder_of("u4")
        self.up = torch.nn.Upsample(scale_factor=2) if how == "module" else torch.nn.UpsamplingNearest2d(size=(8, 10)) if how == "2d" else None
        self.hb = holder_of("u8") if second else None
        self.last = pot_conv(16, 32, 1, 2)
        if two:
            self.pool, self.other = torch.nn.MaxPool2d(2), pot_conv(16, 16, 1, 3)

    def forward(self, x):
        a = self.ha(torch.relu(self.first(self.h0(x))))
        if self.how == "functional":
            u = F.interpolate(a, scale_factor=2.0, mode="nearest-exact")
        elif self.how == "size":
            u = F.interpolate(a, (8, 10))
        else:
            u = self.up(a)
        b = self.hb(u) if self.hb is not None else u
        if self.two:
            return self.last(b)[:, :16, ::2, ::2] + self.other(self.pool(b))
        return self.last(b)


class Decoder(torch.nn.Module):
    """A decoder stage: conv -> ReLU -> A -> Upsample -> B -> cat([B, S]) -> C -> conv3x3, S the holder of the skip input."""

    def __init__(self, geometry=None):
        super().__init__()
        self.h0 = holder_of("s4")
        self.first = pot_conv(16, 16, 1, 1)
        self.ha, self.hb, self.hs, self.hc = holder_of("u4"), holder_of("u8"), holder_of("u2"), holder_of("u4")
        self.up = torch.nn.Upsample(**(geometry or dict(scale_factor=2)))
        self.last = pot_conv(32, 16, 3, 2)

    def forward(self, x, skip):
        b = self.hb(self.up(self.ha(torch.relu(self.first(self.h0(x))))))
        return self.last(self.hc(torch.cat([b, self.hs(skip)], 1)))


def low_input(device="cpu"):
    return (torch.randn(2, 16, 4, 5, generator=torch.Generator().manual_seed(12)) * 1.5).to(device)


def skip_input(device="cpu", size=(8, 10)):
    return (torch.randn(2, 16, *size, generator=torch.Generator().manual_seed(13)).abs() * 0.7).to(device)


ALL = dict(convolutions=True, shared_holders=True, stay_on_codes=True, pools=True, concats=True, muls=True)
SWITCH_SETS = (dict(), dict(convolutions=True), dict(convolutions=True, shared_holders=True), ALL)


def rewritten(make, device="cpu", upsamples=True, **switches):
    from mct_quantizers_amd import consumers
    return consumers.fuse_linear_consumers_fx(make().to(device).eval(), upsamples=upsamples, **switches)


@pytest.mark.parametrize("how", ["module", "2d", "functional", "size"])
def test_a_chain_with_a_second_holder_runs_on_codes(how):
    from mct_quantizers_amd import consumers as C
    x = low_input()
    make = lambda: Chain(True, how)                          # noqa: E731
    with torch.no_grad():
        want = make().eval()(x)
    name = "hb_upsample"
    for switches in SWITCH_SETS:
        gm, n = rewritten(make, **switches)
        gm0, n0 = rewritten(make, upsamples=False, **switches)
        # (a): the upsample and B are one node named after B, the convolution behind a consumer of its codes
        assert name in _targets(gm) and "last_qlinear" in _targets(gm) and "hb" not in _targets(gm) and "up" not in _targets(gm)
        assert F.interpolate not in _targets(gm, "call_function") and not _of(gm0, C.QuantizedUpsample)
        assert n == n0 == (2 if switches.get("convolutions") else 1)      # last is a plain pair behind B without the switch too
        q = gm.get_submodule(name)
        assert q.activation_code_params() == (4.0 / 256, 0, 0, 255) and q.output_code_params() == (8.0 / 256, 0, 0, 255)
        assert gm.get_submodule("last_qlinear").activation_code_params() == q.output_code_params()
        y = gm(x)
        assert y.shape == (2, 32, 8, 10) and len(torch.unique(y)) > 50
        assert torch.equal(y, gm0(x)) and torch.equal(y, want), switches
    # holder A: gone where the upsample alone reads it and nothing is absorbed; a join with shared_holders; with stay_on_codes the
    # convolution in front emits A's codes, the ReLU folded into their clamp
    gm, _ = rewritten(make, convolutions=True)
    assert _targets(gm) == ["first_qlinear", name, "last_qlinear"] and torch.relu in _targets(gm, "call_function")
    gm, _ = rewritten(make, convolutions=True, shared_holders=True)
    assert _targets(gm) == ["first_qlinear", "ha_join", name, "last_qlinear"] and not gm.get_submodule("ha_join").want_float
    gm, _ = rewritten(make, **ALL)
    assert _targets(gm) == ["first_qlinear", name, "last_qlinear"] and torch.relu not in _targets(gm, "call_function")
    first = gm.get_submodule("first_qlinear")
    assert first.emit_codes_for == gm.get_submodule(name).activation_code_params() == (4.0 / 256, 0, 0, 255) and first.emit_clamp is None
    seen = []
    hook = gm.get_submodule(name).register_forward_hook(lambda m, args, out: seen.append((args[0].dtype, tuple(args[0].shape), out.dtype)))
    gm(x)
    hook.remove()
    assert seen == [(torch.uint8, (2, 16, 4, 5), torch.uint8)]
    # tracing the rewritten graph again keeps the node a leaf and replaces nothing more
    again, n = rewritten(lambda: gm, **ALL)
    assert n == 0 and _targets(again) == _targets(gm) and torch.equal(again(x), want)


def test_a_chain_without_a_second_holder_is_a_copy_of_codes():
    from mct_quantizers_amd import consumers as C
    x = low_input()
    make = lambda: Chain(False)                              # noqa: E731
    with torch.no_grad():
        want = make().eval()(x)
    for switches in SWITCH_SETS:
        gm, n = rewritten(make, **switches)
        gm0, n0 = rewritten(make, upsamples=False, **switches)
        # (b): without the switch the convolution behind the upsample reads float32
        assert (n, n0) == ((2, 1) if switches.get("convolutions") else (1, 0))
        assert "up_upsample" in _targets(gm) and "last_qlinear" in _targets(gm) and not _of(gm0, C.QuantizedUpsample)
        q = gm.get_submodule("up_upsample")
        assert q.out_quantizer is None and q.output_code_params() == q.activation_code_params() == (4.0 / 256, 0, 0, 255)
        y = gm(x)
        assert torch.equal(y, gm0(x)) and torch.equal(y, want) and len(torch.unique(y)) > 50


def test_two_readers_and_a_max_pool_behind_the_second_holder():
    from mct_quantizers_amd import consumers as C
    x = low_input()
    make = lambda: Chain(True, two=True)                     # noqa: E731
    with torch.no_grad():
        want = make().eval()(x)
    for switches in (dict(pools=True), dict(convolutions=True, shared_holders=True, pools=True), ALL):
        gm, n = rewritten(make, **switches)
        gm0, n0 = rewritten(make, upsamples=False, **switches)
        assert n == (3 if switches.get("convolutions") else 2) and "hb_upsample" in _targets(gm) and "pool_qpool" in _targets(gm)
        assert "hb" not in _targets(gm) and "hb_join" not in _targets(gm)               # B belongs to the upsample, not to a join
        nodes = {node.target: node for node in gm.graph.nodes if node.op == "call_module"}
        assert sorted(u.target for u in nodes["hb_upsample"].users) == ["last_qlinear", "pool_qpool"]
        assert [u.target for u in nodes["pool_qpool"].users] == ["other_qlinear"]
        assert torch.equal(gm(x), want) and torch.equal(gm0(x), want)
    # without pools the max pool is a float32 reader of B: left alone
    gm, n = rewritten(make, convolutions=True)
    gm0, n0 = rewritten(make, upsamples=False, convolutions=True)
    assert n == n0 and str(gm.graph) == str(gm0.graph) and not _of(gm, C.QuantizedUpsample)


@pytest.mark.parametrize("geometry", [None, dict(size=(7, 9)), dict(scale_factor=(1.75, 2.0), mode="nearest-exact")])
def test_a_decoder_stage_runs_holder_to_holder_on_codes(geometry):
    from mct_quantizers_amd import consumers as C
    x = low_input()
    make = lambda: Decoder(geometry)                         # noqa: E731
    skip = skip_input(size=tuple(make().up(x).shape[2:]))
    with torch.no_grad():
        want = make().eval()(x, skip)
    gm, n = rewritten(make, **ALL)
    gm0, n0 = rewritten(make, upsamples=False, **ALL)
    assert (n, n0) == (2, 2)
    # (c): the concatenation pass absorbed B; the upsample's output was its float32 operand 0 and now is codes of that operand's form
    assert _targets(gm) == ["first_qlinear", "up_upsample", "hc_concat", "last_qlinear"]
    assert _targets(gm0) == ["first_qlinear", "ha", "up", "hc_concat", "last_qlinear"]
    assert not _targets(gm, "call_function") and len(_of(gm, C.QuantizedUpsample)) == 1 and not _of(gm0, C.QuantizedUpsample)
    q, concat, first = gm.get_submodule("up_upsample"), gm.get_submodule("hc_concat"), gm.get_submodule("first_qlinear")
    assert q.output_code_params() == concat.operand_code_params(0) == (8.0 / 256, 0, 0, 255)
    assert first.emit_codes_for == q.activation_code_params() == (4.0 / 256, 0, 0, 255)
    nodes = {node.target: node for node in gm.graph.nodes if node.op == "call_module"}
    assert nodes["hc_concat"].args[0] is nodes["up_upsample"] and nodes["up_upsample"].args == (nodes["first_qlinear"],)
    seen = []
    hook = concat.register_forward_hook(lambda m, args, out: seen.append(([a.dtype for a in args], out.dtype)))
    y = gm(x, skip)
    hook.remove()
    assert seen == [([torch.uint8, torch.float32], torch.uint8)]
    assert torch.equal(y, gm0(x, skip)) and torch.equal(y, want) and len(torch.unique(y)) > 50
    # under fewer switches: the same bits; without concats the float32 torch.cat reads B and everything is left alone
    for switches in (dict(concats=True, convolutions=True), dict(concats=True, convolutions=True, shared_holders=True)):
        gm1, n1 = rewritten(make, **switches)
        assert n1 == 2 and "up_upsample" in _targets(gm1) and torch.equal(gm1(x, skip), want)
    gm2, n2 = rewritten(make, convolutions=True, shared_holders=True, stay_on_codes=True)
    gm20, n20 = rewritten(make, upsamples=False, convolutions=True, shared_holders=True, stay_on_codes=True)
    assert n2 == n20 and str(gm2.graph) == str(gm20.graph) and not _of(gm2, C.QuantizedUpsample)


class Odd(torch.nn.Module):
    """What the switch leaves alone, one at a time."""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind
        self.ha, self.hb = holder_of("u4"), holder_of("u8")
        self.up = {"bilinear": torch.nn.Upsample(scale_factor=2, mode="bilinear"), "bicubic": torch.nn.Upsample(scale_factor=2, mode="bicubic"),
                   "area": torch.nn.Upsample(scale_factor=2, mode="area"), "shuffle": torch.nn.PixelShuffle(2),
                   "transpose": torch.nn.ConvTranspose2d(16, 16, 2, 2), "five_d": torch.nn.Upsample(scale_factor=(2, 2, 2)),
                   "three_d": torch.nn.Upsample(scale_factor=(2,)), "corners": torch.nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True),
                   }.get(kind, torch.nn.Upsample(scale_factor=2))
        self.last = pot_conv(4 if kind == "shuffle" else 16, 16, 1, 1)

    def forward(self, x, other=None):
        a = self.ha(x)
        if self.kind == "antialias":
            u = F.interpolate(a, scale_factor=2, mode="bilinear", antialias=True)
        elif self.kind == "dynamic_size":
            u = F.interpolate(a, size=other.shape[2:])
        else:
            u = self.up(a)
        if self.kind == "activation":
            u = torch.relu(u)
        b = self.hb(u)
        y = self.last(b)
        if self.kind == "float_user_of_b":
            return y + b
        if self.kind == "float_user":                        # FPN: lateral + upsample(top)
            return y + u
        return y


LEFT_ALONE = ["float_user", "float_user_of_b", "bilinear", "bicubic", "area", "corners", "antialias", "dynamic_size", "shuffle", "transpose",
              "three_d", "five_d", "activation"]


@pytest.mark.parametrize("kind", LEFT_ALONE)
def test_what_the_switch_leaves_alone(kind):
    from mct_quantizers_amd import consumers as C
    for switches in (dict(), dict(convolutions=True, shared_holders=True), ALL):
        gm, n = C.fuse_linear_consumers_fx(Odd(kind).eval(), upsamples=True, **switches)
        gm0, n0 = C.fuse_linear_consumers_fx(Odd(kind).eval(), **switches)
        assert n == n0 and not _of(gm, C.QuantizedUpsample), (kind, switches)
        assert str(gm.graph) == str(gm0.graph) and gm.code == gm0.code
    if kind not in ("three_d", "five_d"):                    # (those two describe no 4-D upsample: they cannot run)
        x = skip_input(size=(4, 5))
        args = (x, skip_input()) if kind == "dynamic_size" else (x,)
        with torch.no_grad():
            assert torch.equal(gm(*args), Odd(kind).eval()(*args))


def test_without_the_keyword_nothing_changes():
    from mct_quantizers_amd import consumers as C
    for switches in SWITCH_SETS:
        for make in (Chain, lambda: Chain(False), Decoder):
            gm, n = C.fuse_linear_consumers_fx(make().eval(), **switches)
            gm_off, n_off = C.fuse_linear_consumers_fx(make().eval(), upsamples=False, **switches)
            assert n == n_off and str(gm.graph) == str(gm_off.graph) and gm.code == gm_off.code
            assert not _of(gm, C.QuantizedUpsample)


def sequential(second=True):
    from test_pool_consumer import pot_holder
    layers = [pot_holder(True), pot_conv(16, 16, 3, 1), holder_of("u4"), torch.nn.Upsample(scale_factor=2)]
    return torch.nn.Sequential(*layers, *([holder_of("u8")] if second else []), pot_conv(16, 32, 1, 2)).eval()


@pytest.mark.parametrize("second", [True, False])
def test_sequential_rewrite(second):
    from mct_quantizers_amd import consumers as C
    plain, fused, chained = sequential(second), sequential(second), sequential(second)
    assert C.fuse_linear_consumers(plain, convolutions=True) == (2 if second else 1)
    assert C.fuse_linear_consumers(fused, convolutions=True, upsamples=True) == 2
    assert C.fuse_linear_consumers(chained, convolutions=True, upsamples=True, chain=True) == 2
    gap = [C._FusedAway] if second else []
    assert [type(m) for m in fused] == [C._FusedAway, C.QuantizedConv2d, C._FusedAway, C.QuantizedUpsample, *gap, C.QuantizedConv1x1]
    assert not [m for m in plain if isinstance(m, C.QuantizedUpsample)] and type(plain[3]) is torch.nn.Upsample
    assert fused[3].output_code_params() == fused[-1].activation_code_params() == ((8.0 / 256 if second else 4.0 / 256), 0, 0, 255)
    assert chained[1].emit_codes_for == chained[3].activation_code_params() == (4.0 / 256, 0, 0, 255) and fused[1].emit_codes_for is None
    x = low_input().abs()
    with torch.no_grad():
        want = sequential(second)(x)
    assert torch.equal(fused(x), want) and torch.equal(plain(x), want) and torch.equal(chained(x), want)
    assert want.shape == (2, 32, 8, 10) and len(torch.unique(want)) > 50
    # a bilinear upsample, and a Linear behind (rows): left alone
    other = sequential(second)
    other[3] = torch.nn.Upsample(scale_factor=2, mode="bilinear")
    assert C.fuse_linear_consumers(other, convolutions=True, upsamples=True) == (2 if second else 1)
    assert not [m for m in other if isinstance(m, C.QuantizedUpsample)]


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------

def check_refusals(lib, native, P=4096):
    """Every refusal of mctq_codes_upsample_nhwc: each returns before a launch (the addresses are never dereferenced), so none
    can fault.  ``P``: an aligned address, on the GPU that of a real buffer of at least 8 KiB."""
    E, I8, U8 = native.MCTQ_E_ARG, native.CODE_I8, native.CODE_U8
    count, last = lib.mctq_launch_count(), lib.mctq_last_launch()
    Q, R = P + 4096, P + 6144                                 # the codes' address and the maps'; out at P: 2 * 4 * 4 * 16 bytes

    def call(codes=Q, out=P, dt=U8, in_zp=3, in_scale=0.1, b=2, h=2, w=2, c=16, ho=4, wo=4, fh=2, fw=2, rows=None, cols=None,
             odt=I8, scale=0.05, zp=-3, qmin=-128, qmax=127):
        return lib.mctq_codes_upsample_nhwc(codes, out, dt, in_zp, in_scale, b, h, w, c, ho, wo, fh, fw, rows, cols, odt, scale, zp,
                                            qmin, qmax, None)

    def refused(message, **fault):
        assert call(**fault) == E, fault
        assert lib.mctq_last_error() == message, (fault, lib.mctq_last_error())

    mapped = dict(fh=0, fw=0, rows=R, cols=R + 64)
    for extent in ("b", "h", "w", "c", "ho", "wo"):
        refused(b"negative extent", **{extent: -1})
    for channels in (24, 8, 1):
        refused(b"channels must be a multiple of 16", c=channels)
    for dt in (-1, 2, 3, 77):                                # the 4-bit code types among them
        refused(b"bad code_dtype", dt=dt)
        refused(b"bad out_code_dtype", odt=dt)
    for dt, zp in ((U8, -1), (U8, 256), (I8, -129), (I8, 128)):
        refused(b"in_zero_point is no code of the input's type", dt=dt, in_zp=zp)
    refused(b"zero_point is no code of the output's type", zp=128)
    refused(b"zero_point is no code of the output's type", zp=-129)
    refused(b"zero_point is no code of the output's type", odt=U8, qmin=0, qmax=255, zp=-1)
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        refused(b"in_scale must be finite and positive", in_scale=bad)
        refused(b"scale must be finite and positive", scale=bad)
    refused(b"quant_min > quant_max", qmin=9, qmax=8)
    refused(b"clamp domain does not fit the code type", qmax=128)
    refused(b"clamp domain does not fit the code type", odt=U8, zp=3, qmin=-1, qmax=255)
    refused(b"clamp domain does not fit the code type", qmin=0, qmax=255)
    either = b"give either src_rows and src_cols (factors 0) or factor_h and factor_w (maps NULL)"
    refused(either, rows=R, cols=R + 64)                      # both
    refused(either, rows=R)
    refused(either, fh=0, fw=0)                               # neither
    refused(b"src_rows and src_cols go together", fh=0, fw=0, rows=R)
    refused(b"src_rows and src_cols go together", fh=0, fw=0, cols=R)
    refused(b"factor_h and factor_w must be at least 1", fh=0)
    refused(b"factor_h and factor_w must be at least 1", fw=-2)
    refused(b"an image extent exceeds 2^31 - 1", h=2 ** 31, ho=2 ** 32)
    refused(b"an image extent exceeds 2^31 - 1", wo=2 ** 31, **mapped)
    mismatch = b"out_height / out_width are not factor_h * height / factor_w * width"
    refused(mismatch, ho=5)
    refused(mismatch, wo=2)
    refused(mismatch, fh=3)
    refused(mismatch, fh=1, fw=1)
    refused(b"a non-empty output needs an image of at least one pixel", h=0, **mapped)
    refused(b"a non-empty output needs an image of at least one pixel", w=0, **mapped)
    refused(b"more than 2^31 - 1 16-byte chunks of output in one launch", b=2 ** 27)     # 2^27 * 16 pixels of one chunk
    refused(b"more than 2^31 - 1 16-byte chunks of output in one launch", c=16 * 2 ** 26)
    refused(b"more than 2^31 - 1 16-byte chunks of output in one launch", b=2 ** 62)
    refused(b"more than 2^31 - 1 16-byte chunks of output in one launch", ho=2 ** 20, wo=2 ** 20, **mapped)
    refused(b"the input's byte count exceeds 2^62", b=2 ** 20, h=2 ** 30, w=2 ** 30, ho=1, wo=1, **mapped)
    refused(b"NULL pointer", codes=None)
    refused(b"NULL pointer", out=None)
    refused(b"codes and out must be 16-byte aligned", codes=Q + 8)
    refused(b"codes and out must be 16-byte aligned", out=P + 4)
    refused(b"src_rows and src_cols must be 4-byte aligned", fh=0, fw=0, rows=R + 2, cols=R + 64)
    refused(b"src_rows and src_cols must be 4-byte aligned", fh=0, fw=0, rows=R, cols=R + 65)
    # out overlapping the codes: the same address, the codes' last byte, out's last byte
    refused(b"out overlaps codes", codes=P)
    refused(b"out overlaps codes", codes=P - 112)
    refused(b"out overlaps codes", codes=P + 496)
    refused(b"out overlaps a map", fh=0, fw=0, rows=P + 508, cols=R)
    refused(b"out overlaps a map", fh=0, fw=0, rows=R, cols=P - 12)
    # wrong in two ways: the extents, the channels, the input's form, the output's form, the map, the geometry, the pointers
    refused(b"negative extent", b=-1, c=8)
    refused(b"channels must be a multiple of 16", c=8, dt=77)
    refused(b"bad code_dtype", dt=77, in_zp=999, odt=77)
    refused(b"in_scale must be finite and positive", in_scale=0.0, odt=77)
    refused(b"bad out_code_dtype", odt=77, qmin=9, qmax=8)
    refused(b"scale must be finite and positive", scale=0.0, qmin=9, qmax=8)
    refused(b"quant_min > quant_max", qmin=9, qmax=8, fh=0)
    refused(b"factor_h and factor_w must be at least 1", fh=0, ho=5)
    refused(mismatch, ho=5, codes=None)
    # nothing to do: no launch, and no pointer is looked at
    assert call(b=0) == 0 and call(c=0) == 0 and call(h=0, ho=0) == 0 and call(w=0, wo=0) == 0
    assert call(b=0, codes=None, out=None) == 0 and call(ho=0, **mapped) == 0 and call(wo=0, codes=None, **mapped) == 0
    refused(b"channels must be a multiple of 16", b=0, c=8)
    for value in (3, -1):
        assert lib.mctq_set_tuning(b"upsample_form", value) == E
        assert lib.mctq_last_error() == b"upsample_form must be 0 (auto), 1 (gather) or 2 (replicate)"
    assert lib.mctq_launch_count() == count and lib.mctq_last_launch() == last             # refused and empty calls launch nothing


def test_codes_upsample_argument_validation_needs_no_gpu():
    import os
    import re
    from conftest import REPO
    from mct_quantizers_amd.hip import build, native
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    lib = native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mctq_hip.h")).read(), flags=re.S)
    assert re.search(r"\bmctq_codes_upsample_nhwc\s*\(", header) and "mctq_codes_upsample_nhwc" in native.SIGNATURES
    assert lib.mctq_abi_version() == 10 == native.ABI_VERSION
    assert "mctq_codes_upsample.hip" in [os.path.basename(s) for s in build.SOURCES]
    assert "mctq_codes_upsample_nhwc" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    for value in (1, 2, 0):
        assert lib.mctq_set_tuning(b"upsample_form", value) == 0
    check_refusals(lib, native)
