"""Integer consumer for LUT (codebook) weights without a GPU (consumers.QuantizedLinear with WeightsLUTSymmetric /
WeightsLUTPOT quantizers, consumers.pack_lut4, mctq_qlinear_lut4a8's argument validation).

A LUT-quantized weight with int8 codebook values is an int8 times a per-row scale,
    q(w)[n][k] = (lut[idx] / 2^(B-1)) * thr[n] == float(lut_i8[idx]) * (thr[n] / 2^(B-1))       (bit for bit),
so the oracle is the integer consumer's own (oracle/mctq_oracle.py::qlinear_i8) on lut_i8[idx] with scales thr / 128.
"""
import os
import re
import warnings

import numpy as np
import pytest
import torch

from conftest import REPO, bits_equal, first_mismatch

K, N = 64, 24

CODEBOOKS = {
    "16": [-120.0, 77.0, -2.0, 38.0, -96.0, 3.0, 127.0, -50.0, 11.0, -33.0, 100.0, -9.0, 24.0, -70.0, 55.0, -20.0],
    "8": [22.0, -53.0, 62.0, 0.0, -66.0, -21.0, 44.0, -40.0],
    "3dup": [3.0, 3.0, -8.0],
    "extremes": [-128.0, 127.0, 0.0, -64.0, 63.0, 17.0],
    "32": [float(v) for v in (np.arange(32) * 8 - 125)[np.random.default_rng(5).permutation(32)]],
}
BITS = {"16": 4, "8": 3, "3dup": 2, "extremes": 3, "32": 5}


def _weights_quantizer(lin_weight, codebook, kind, per_channel, channel_axis=0, bitwidth=8, rank=2):
    import mct_quantizers_amd as mq
    Q = mq.pytorch_quantizers
    lut = CODEBOOKS[codebook]
    n = lin_weight.shape[0]
    if kind == "pot":
        cls = Q.WeightsLUTPOTInferableQuantizer
        thr = [float(2.0 ** (-3 + i % 3)) for i in range(n)] if per_channel else [0.25]
    else:
        cls = Q.WeightsLUTSymmetricInferableQuantizer
        thr = [float(v) for v in lin_weight.detach().reshape(n, -1).abs().max(1).values] if per_channel \
            else [float(lin_weight.detach().abs().max())]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cls(num_bits=BITS[codebook], lut_values=lut, threshold=thr, per_channel=per_channel,
                   channel_axis=channel_axis if per_channel else None, input_rank=rank if per_channel else None,
                   lut_values_bitwidth=bitwidth)


def _activation_quantizer(act):
    import mct_quantizers_amd as mq
    Q = mq.pytorch_quantizers
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if act == "uniform":
            return Q.ActivationUniformInferableQuantizer(num_bits=8, min_range=[-2.5], max_range=[3.1])
        if act == "signed":
            return Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[3.3], signed=True)
        return Q.ActivationPOTInferableQuantizer(num_bits=8, threshold=[4.0], signed=False)


def lut_model(k=K, n=N, codebook="16", kind="sym", per_channel=True, act="uniform", seed=0, **kw):
    """holder -> wrapped Linear(k, n) with a LUT weights quantizer (tests/test_consumers.py::_model's LUT twin)."""
    import mct_quantizers_amd as mq
    torch.manual_seed(seed)
    lin = torch.nn.Linear(k, n)
    wq = _weights_quantizer(lin.weight, codebook, kind, per_channel, **kw)
    return torch.nn.Sequential(mq.PytorchActivationQuantizationHolder(_activation_quantizer(act)),
                               mq.PytorchQuantizationWrapper(lin, {"weight": wq}))


def lut_operands(wq, weight):
    """(lut_i8[idx] int8 [N, K], thr / 2^(B-1) float32 [N], idx) of a LUT weights quantizer, computed independently of
    consumers.py from the quantizer's own codes."""
    idx, lut, thr = wq.quantize_to_codes(weight.detach())
    n = weight.shape[0]
    idx = idx.cpu().numpy().reshape(n, -1)
    lut_i8 = lut.cpu().numpy().astype(np.int8)
    assert np.array_equal(lut_i8.astype(np.float32), lut.cpu().numpy())
    ws = thr.cpu().numpy().astype(np.float32) / np.float32(2.0 ** (wq.lut_values_bitwidth - 1))
    ws = np.broadcast_to(ws, (n,)).astype(np.float32) if ws.size == 1 else ws
    return lut_i8[idx], ws, idx


def test_pack_lut4_round_trips_against_the_documented_layout():
    from mct_quantizers_amd import consumers
    idx = torch.randint(0, 16, (5, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    idx[0, :16] = torch.arange(16, dtype=torch.uint8)
    packed = consumers.pack_lut4(idx)
    assert packed.shape == (5, 16) and packed.dtype == torch.uint8 and packed.is_contiguous()
    b = packed.numpy().reshape(5, 4, 4)                               # [row][group of 8 k][byte j]
    back = np.empty((5, 4, 8), np.uint8)
    for j in range(4):
        back[:, :, j] = b[:, :, j] & 0xF                              # k = j
        back[:, :, j + 4] = b[:, :, j] >> 4                           # k = j + 4
    assert np.array_equal(back.reshape(5, 32), idx.numpy())
    assert packed[0, :4].tolist() == [0x40, 0x51, 0x62, 0x73]
    with pytest.raises(ValueError):
        consumers.pack_lut4(torch.full((2, 8), 16, dtype=torch.uint8))
    with pytest.raises(ValueError):
        consumers.pack_lut4(torch.zeros((2, 12), dtype=torch.uint8))
    with pytest.raises(ValueError):
        consumers.pack_lut4(torch.zeros((2, 8), dtype=torch.int8))


@pytest.mark.parametrize("act", ["uniform", "signed", "unsigned_pot"])
@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("kind", ["sym", "pot"])
@pytest.mark.parametrize("codebook", list(CODEBOOKS))
def test_fused_lut_linear_on_cpu_matches_oracle_and_reference_path(codebook, kind, per_channel, act):
    from oracle import mctq_oracle as O
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    model = lut_model(codebook=codebook, kind=kind, per_channel=per_channel, act=act)
    wq, weight = model[1].weights_quantizers["weight"], model[1].weight
    x = torch.randn(3, 5, K, generator=torch.Generator().manual_seed(7)) * 1.5
    ref = model(x)                                                  # fused fake-quant + float32 F.linear
    w_codes, ws, idx = lut_operands(wq, weight)
    # the scale identity the consumer rests on: int8 codebook value times thr / 128 is the fake-quantized weight
    assert bits_equal(w_codes.astype(np.float32) * ws[:, None], wq(weight.detach().clone()).cpu().numpy())
    if codebook == "3dup":
        assert set(np.unique(idx)) <= {0, 2}                        # the duplicate's first occurrence
    assert consumers.fuse_linear_consumers(model) == 1
    ql = model[1]
    assert isinstance(model[0], torch.nn.Identity) and isinstance(ql, consumers.QuantizedLinear)
    y = model(x)
    assert y.shape == ref.shape == (3, 5, N)
    a_codes = ops.fq_codes(x.reshape(-1, K), None, None, None, ql._a_qmin, ql._a_qmax, ql._a_scale, ql._a_zp)
    want = O.qlinear_i8(a_codes.numpy(), ql._a_zp, ql._a_scale, w_codes, ws, ql.bias.detach().numpy())
    got = y.detach().reshape(-1, N).numpy()
    assert bits_equal(got, want), first_mismatch(got, want)
    err = float((y - ref).detach().abs().max()) / float(ref.detach().abs().max())
    print(f"{codebook} {kind} per_channel={per_channel} {act}: max |y - ref| / max |ref| = {err:.3g}")
    assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))
    assert np.array_equal(ql._w_codes.numpy(), w_codes) and bits_equal(ql._w_scales.numpy(), ws)
    assert ql._w_idx4 is None                                       # packed indices are kept for GPU weights only


def test_extreme_codebook_values_reach_the_product():
    """Weights beyond the thresholds quantize to the codebook's -128 and 127: the fused layer still equals the oracle."""
    from oracle import mctq_oracle as O
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    model = lut_model(codebook="extremes", kind="pot", per_channel=True)
    with torch.no_grad():
        model[1].weight.mul_(8.0)
    w_codes, ws, _ = lut_operands(model[1].weights_quantizers["weight"], model[1].weight)
    assert w_codes.min() == -128 and w_codes.max() == 127
    x = torch.randn(6, K, generator=torch.Generator().manual_seed(2)) * 2.0
    ref = model(x)
    assert consumers.fuse_linear_consumers(model) == 1
    ql = model[1]
    y = model(x)
    a_codes = ops.fq_codes(x, None, None, None, ql._a_qmin, ql._a_qmax, ql._a_scale, ql._a_zp)
    want = O.qlinear_i8(a_codes.numpy(), ql._a_zp, ql._a_scale, w_codes, ws, ql.bias.detach().numpy())
    assert bits_equal(y.detach().numpy(), want)
    assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))


def test_fuse_leaves_lut_pairs_it_cannot_take_alone():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    wide = lut_model(codebook="16", bitwidth=10)                                   # codebook values wider than int8
    assert consumers.fuse_linear_consumers(wide) == 0 and isinstance(wide[1], mq.PytorchQuantizationWrapper)
    other_axis = lut_model(k=32, n=32, codebook="16", channel_axis=1)              # thresholds along the input channels
    assert consumers.fuse_linear_consumers(other_axis) == 0
    odd = lut_model(k=24, n=8, codebook="16")                                      # K % 16 != 0
    assert consumers.fuse_linear_consumers(odd) == 0
    with pytest.raises(NotImplementedError):
        consumers.QuantizedLinear(wide[1].layer, wide[1].weights_quantizers["weight"], _activation_quantizer("signed"))
    with pytest.raises(NotImplementedError):
        consumers.QuantizedLinear(other_axis[1].layer, other_axis[1].weights_quantizers["weight"],
                                  _activation_quantizer("signed"))
    x = torch.randn(2, 32)
    assert other_axis(x).shape == (2, 32)                                          # the unfused pair still runs


def test_lut_weight_codes_follow_in_place_weight_updates():
    from mct_quantizers_amd import consumers
    model = lut_model()
    assert consumers.fuse_linear_consumers(model) == 1
    ql = model[1]
    x = torch.randn(4, K)
    y0 = model(x)
    codes0, rowsum0 = ql._w_codes.clone(), ql._w_rowsum.clone()
    with torch.no_grad():
        ql.weight.mul_(0.5)
    y1 = model(x)
    assert not torch.equal(codes0, ql._w_codes) and not torch.equal(y0, y1)
    assert torch.equal(ql._w_rowsum, ql._w_codes.sum(dim=1, dtype=torch.int32)) and not torch.equal(rowsum0, ql._w_rowsum)
    w_codes, ws, _ = lut_operands(ql.weights_quantizer, ql.weight)
    assert np.array_equal(ql._w_codes.numpy(), w_codes)


def test_pointwise_convolution_with_lut_weights_fuses():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(32, 16, 1)
    wq = _weights_quantizer(conv.weight, "16", "sym", True, rank=4)

    def build():
        c = torch.nn.Conv2d(32, 16, 1)
        c.load_state_dict(conv.state_dict())
        return torch.nn.Sequential(mq.PytorchActivationQuantizationHolder(_activation_quantizer("uniform")),
                                   mq.PytorchQuantizationWrapper(c, {"weight": wq}))
    ref_model, model = build(), build()
    assert consumers.fuse_linear_consumers(model) == 1 and isinstance(model[1], consumers.QuantizedConv1x1)
    for fmt in (torch.contiguous_format, torch.channels_last):
        x = (torch.randn(2, 32, 7, 5) * 1.5).contiguous(memory_format=fmt)
        ref, y = ref_model(x), model(x)
        assert y.shape == ref.shape == (2, 16, 7, 5)
        assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))


def test_fx_rewrite_takes_a_lut_pair():
    from mct_quantizers_amd import consumers

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            m = lut_model(codebook="8", kind="pot")
            self.h, self.l = m[0], m[1]

        def forward(self, x):
            return torch.relu(self.l(self.h(x))) + 1.0

    net = Net()
    x = torch.randn(9, K) * 1.5
    ref = net(x)
    gm, n = consumers.fuse_linear_consumers_fx(net)
    assert n == 1 and [type(m).__name__ for m in gm.modules()].count("QuantizedLinear") == 1
    y = gm(x)
    assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))


def test_chained_lut_layers_pass_codes_on_cpu():
    from mct_quantizers_amd import consumers

    def stack():
        a, b = lut_model(k=64, n=64, codebook="16", seed=1, act="uniform"), lut_model(k=64, n=32, codebook="8", kind="pot",
                                                                                      seed=2, act="signed")
        return torch.nn.Sequential(a[0], a[1], b[0], b[1])
    plain, chained = stack(), stack()
    assert consumers.fuse_linear_consumers(plain) == 2 and consumers.fuse_linear_consumers(chained, chain=True) == 2
    x = torch.randn(7, 64) * 1.5
    assert chained[1].emit_codes_for is not None and chained[:2](x).dtype == torch.int8
    assert torch.equal(plain(x), chained(x))


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from mct_quantizers_amd.hip import build, native
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    return native.load()


def test_lut4a8_symbol_and_argument_validation(lib):
    import ctypes
    from mct_quantizers_amd.hip import build, native
    E, U8, I8 = native.MCTQ_E_ARG, native.CODE_U8, native.CODE_I8
    text = open(os.path.join(REPO, "include", "mctq_hip.h")).read()
    assert re.search(r"\bint mctq_qlinear_lut4a8\(", text) and "mctq_qlinear_lut4a8" in native.SIGNATURES
    assert hasattr(ctypes.CDLL(build.OUT), "mctq_qlinear_lut4a8")
    assert lib.mctq_abi_version() == 10 == native.ABI_VERSION          # the export is additive
    assert len(native.SIGNATURES["mctq_qlinear_lut4a8"][1]) == len(native.SIGNATURES["mctq_qlinear_w4a8"][1]) + 1
    f = lib.mctq_qlinear_lut4a8
    P = 0x1000                                  # an aligned non-NULL address: validation dereferences nothing
    lut = bytes(range(16))

    def err(rc, msg):
        assert rc == E, rc
        assert msg in lib.mctq_last_error(), lib.mctq_last_error()

    def call(a=P, adt=I8, w=P, lut16=lut, ydt=-1, M=4, N=8, Kk=64, y=P):
        return f(a, adt, 0, 1.0, w, lut16, P, P, None, y, ydt, 1.0, 0, -128, 127, M, N, Kk, None)

    err(call(M=-1), b"negative extent")
    err(call(N=-3), b"negative extent")
    err(call(Kk=24), b"multiple of 16")
    err(call(Kk=32768 + 16), b"32768")
    err(call(lut16=None), b"lut16 is NULL")
    err(call(w=None), b"NULL pointer")
    err(call(a=None), b"NULL pointer")
    err(call(a=P + 8), b"aligned")
    err(call(w=P + 4), b"aligned")
    err(call(ydt=7), b"bad y_code_dtype")
    err(call(adt=9), b"bad a_code_dtype")
    err(f(P, I8, 0, 1.0, P, lut, P, P, None, P, U8, 1.0, 0, -5, 300, 4, 8, 64, None), b"clamp domain")
    count = lib.mctq_launch_count()
    assert call(M=0, a=None, w=None, y=None) == 0                       # empty products launch nothing
    assert call(N=0, a=None, w=None, y=None) == 0
    assert lib.mctq_launch_count() == count
    # the 4-bit codes entry point shares the validation and keeps its behaviour
    g = lib.mctq_qlinear_w4a8
    assert g(P, I8, 0, 1.0, P + 4, P, P, None, P, -1, 1.0, 0, 0, 0, 4, 8, 64, None) == E and b"aligned" in lib.mctq_last_error()
    assert g(P, I8, 0, 1.0, None, P, P, None, P, -1, 1.0, 0, 0, 0, 4, 8, 64, None) == E
    assert g(None, I8, 0, 1.0, None, None, None, None, None, -1, 1.0, 0, 0, 0, 0, 8, 64, None) == 0


def test_lut16_host_bytes():
    from mct_quantizers_amd import consumers
    assert consumers._lut16_bytes([3.0, 3.0, -8.0]) == bytes([3, 3, 0xF8] + [0] * 13)
    assert consumers._lut16_bytes(torch.tensor([-128, 127], dtype=torch.int8)) == bytes([0x80, 0x7F] + [0] * 14)
    assert consumers._lut16_bytes(bytes(range(16))) == bytes(range(16))
    for bad in ([0.5], [128.0], list(range(17)), b"short"):
        with pytest.raises(ValueError):
            consumers._lut16_bytes(bad)
