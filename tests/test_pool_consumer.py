"""Max pooling on activation codes: host logic and the CPU route (include/mctq_hip.h: mctq_codes_maxpool_nhwc; hip/ops.py:
codes_maxpool; consumers.QuantizedMaxPool2d and the ``pools`` switch of fuse_linear_consumers / fuse_linear_consumers_fx).

Everything here is exact, so every check is equality.  A holder's float32 output is ``float(code - zp) * scale`` with
``scale > 0``, monotone non-decreasing in the code and never NaN: the pool of the dequantized codes is the dequantized pool of
the codes.  The op is pinned against plain numpy loops in which a tap outside the image is skipped (it stands for -inf), and
against ``F.max_pool2d`` of the codes.

A model rewritten with ``pools=True`` is compared bit for bit with the same rewrite without it.  Without the switch the
convolutions behind a pool stay float32 wrappers, so the test models are built so that their float32 products are exact too:
power-of-two activation and weight scales, no bias, and sums of at most 288 products of |a| <= 255 and |w| <= 128 (below 2^24
units of the product of the two scales) -- every partial sum of the float32 convolution is then representable, whatever its
order, and equals the consumer's integer sum times the scales."""
import functools
import operator
import warnings

import numpy as np
import pytest
import torch

from test_conv_consumer import weights_quantizer
from test_join_consumer import _targets

F = torch.nn.functional

# (kernel, stride, padding, dilation, ceil_mode), each on B=2 images of 7 x 5 with 16 and 48 channels: windows over the top / left
# edge; over the bottom / right edge; the dropped last window (7 + 1 <= 4 * 2 and 5 + 1 <= 3 * 2); gaps between windows; a
# rectangular kernel with rectangular stride and padding; dilation with and without padding; the identity
GEOMETRIES = [((3, 3), (2, 2), (1, 1), (1, 1), False), ((3, 3), (2, 2), (1, 1), (1, 1), True), ((2, 2), (2, 2), (0, 0), (1, 1), True),
              ((2, 2), (2, 2), (1, 1), (1, 1), True), ((2, 2), (3, 3), (0, 0), (1, 1), False), ((3, 2), (2, 3), (1, 0), (1, 1), False),
              ((2, 2), (1, 1), (0, 0), (2, 2), False), ((3, 3), (1, 1), (1, 1), (2, 2), False), ((1, 1), (1, 1), (0, 0), (1, 1), False)]
# about 300 output pixels of 3 chunks: several 256-lane blocks, the last one partly empty
LARGE = (3, 20, 20, 48, ((2, 2), (2, 2), (0, 0), (1, 1), False))
PARAMS = [(0.031, 0, 0, 255), (0.022, 114, 0, 255), (0.027, -5, -128, 127)]          # (scale, zero point, qmin, qmax)


def out_size(n, k, s, p, d, ceil_mode):
    """PyTorch's pooling_output_shape, written out independently of ops._pool_out_size."""
    num = n + 2 * p - d * (k - 1) - 1 + (s - 1 if ceil_mode else 0)
    out = num // s + 1
    if ceil_mode and (out - 1) * s >= n + p:
        out -= 1
    return out


def maxpool_loops(codes, k, s, p, d, ceil_mode):
    """codes [B, H, W, C] -> [B, Ho, Wo, C] by plain loops; taps outside the image are skipped."""
    B, H, W, C = codes.shape
    ho, wo = out_size(H, k[0], s[0], p[0], d[0], ceil_mode), out_size(W, k[1], s[1], p[1], d[1], ceil_mode)
    out = np.zeros((B, ho, wo, C), dtype=codes.dtype)
    for oy in range(ho):
        for ox in range(wo):
            taps = [codes[:, iy, ix] for iy in range(oy * s[0] - p[0], oy * s[0] - p[0] + d[0] * k[0], d[0]) if 0 <= iy < H
                    for ix in range(ox * s[1] - p[1], ox * s[1] - p[1] + d[1] * k[1], d[1]) if 0 <= ix < W]
            assert taps                                  # every window of these geometries has a tap inside the image
            out[:, oy, ox] = np.max(np.stack(taps), axis=0)
    return out


@functools.lru_cache(maxsize=None)
def pool_case(u8, C, geometry, B=2, H=7, W=5):
    """(codes [B, H, W, C], the loops' result), computed once and shared by the CPU and GPU tests; read-only.  uint8: the whole
    range, so that codes >= 128 sit next to small ones (the compare must not be signed).  int8: image 0 the whole range, the
    last image negative throughout (neither a padded tap nor the start of the maximum nor a tap of image 0 may win)."""
    rng = np.random.default_rng(100 * C + 7 * H + u8)
    if u8:
        codes = rng.integers(0, 256, (B, H, W, C)).astype(np.uint8)
    else:
        codes = rng.integers(-128, 128, (B, H, W, C)).astype(np.int8)
        codes[-1] = rng.integers(-128, 0, (H, W, C)).astype(np.int8)
    want = maxpool_loops(codes, *geometry)
    codes.setflags(write=False)
    want.setflags(write=False)
    return codes, want


def pool_cases():
    for u8 in (True, False):
        for C in (16, 48):
            for g in GEOMETRIES:
                yield u8, C, g, {}
        B, H, W, C, g = LARGE
        yield u8, C, g, dict(B=B, H=H, W=W)


# ---- the op ----------------------------------------------------------------------------------------------------------------

def test_codes_maxpool_on_cpu_equals_the_loops_and_max_pool2d_of_the_codes():
    from mct_quantizers_amd.hip import ops
    n = 0
    for u8, C, g, shape in pool_cases():
        codes, want = pool_case(u8, C, g, **shape)
        k, s, p, d, ceil_mode = g
        x = torch.from_numpy(codes.copy())
        got = ops.codes_maxpool(x, k, s, p, d, ceil_mode)
        aten = F.max_pool2d(x.permute(0, 3, 1, 2).contiguous(), k, s, p, d, ceil_mode)
        assert got.dtype == x.dtype and got.is_contiguous() and tuple(got.shape) == want.shape, (g, got.shape)
        assert tuple(got.shape) == (aten.shape[0], aten.shape[2], aten.shape[3], aten.shape[1])
        assert np.array_equal(got.numpy(), want) and torch.equal(got.permute(0, 3, 1, 2), aten), (u8, C, g)
        if not u8:
            assert int(got[-1].max()) < 0 and int(got[0].max()) > 100
        n += 1
    assert n == 2 * (2 * len(GEOMETRIES) + 1)
    x = torch.from_numpy(pool_case(True, 16, GEOMETRIES[0])[0].copy())
    assert torch.equal(ops.codes_maxpool(x, 2), ops.codes_maxpool(x, (2, 2), (2, 2), 0, 1, False))      # stride None: the kernel size
    assert torch.equal(ops.codes_maxpool(x, 3, padding=1), ops.codes_maxpool(x, 3, 3, 1))
    nhwc_view = x.permute(0, 2, 1, 3)                                                                    # not contiguous
    assert torch.equal(ops.codes_maxpool(nhwc_view, 2), ops.codes_maxpool(nhwc_view.contiguous(), 2))
    assert ops.codes_maxpool(x[:0], 2).shape == (0, 3, 2, 16)


def test_codes_maxpool_validation():
    from mct_quantizers_amd.hip import ops
    x = torch.zeros(2, 7, 5, 16, dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        ops.codes_maxpool(x.float(), 2)
    with pytest.raises(NotImplementedError):
        ops.codes_maxpool(x.to(torch.int16), 2)
    with pytest.raises(ValueError, match="codes_maxpool takes"):
        ops.codes_maxpool(x[0], 2)
    with pytest.raises(ValueError, match="larger than half"):
        ops.codes_maxpool(x, 2, 1, 2)
    with pytest.raises(ValueError, match="larger than half"):
        ops.codes_maxpool(x, (3, 2), 1, (1, 2))
    with pytest.raises(ValueError, match="codes_maxpool: kernel_size must be an int or a pair"):
        ops.codes_maxpool(x, (2, 2, 2))
    with pytest.raises(ValueError, match="codes_maxpool: stride must be an int or a pair"):
        ops.codes_maxpool(x, 2, (1.5, 1))
    with pytest.raises(ValueError, match="codes_maxpool: padding must be an int or a pair"):
        ops.codes_maxpool(x, 2, 2, (0,))
    for bad in (dict(kernel_size=0), dict(kernel_size=2, stride=0), dict(kernel_size=2, dilation=0), dict(kernel_size=2, padding=-1)):
        with pytest.raises(ValueError, match="at least"):
            ops.codes_maxpool(x, **bad)
    with pytest.raises(ValueError, match="does not fit"):
        ops.codes_maxpool(x, 6)                            # 6 > 5


@pytest.mark.parametrize("params", PARAMS)
def test_dequantize_commutes_with_the_pool(params):
    from mct_quantizers_amd.hip import ops
    scale, zp, qmin, qmax = params
    n = 0
    for u8, C, g, shape in pool_cases():
        if u8 != (qmin == 0):
            continue
        k, s, p, d, ceil_mode = g
        c = torch.from_numpy(pool_case(u8, C, g, **shape)[0].copy())
        pooled_then_dequantized = ops.dequantize_codes(ops.codes_maxpool(c, k, s, p, d, ceil_mode), scale, zp)
        dequantized_then_pooled = F.max_pool2d(ops.dequantize_codes(c, scale, zp).permute(0, 3, 1, 2), k, s, p, d, ceil_mode)
        assert torch.equal(pooled_then_dequantized.permute(0, 3, 1, 2), dequantized_then_pooled), (params, C, g)
        n += 1
    assert n == 2 * len(GEOMETRIES) + 1


def test_output_size_helper_equals_max_pool2d():
    from mct_quantizers_amd.hip import ops
    n = refused = 0
    for size in range(1, 13):
        x = torch.zeros(1, 1, size, 1)
        for k in range(1, 5):
            for s in range(1, 5):
                for p in range(0, k // 2 + 1):
                    for d in (1, 2):
                        for ceil_mode in (False, True):
                            got = ops._pool_out_size(size, k, s, p, d, ceil_mode)
                            assert got == out_size(size, k, s, p, d, ceil_mode)
                            try:
                                want = F.max_pool2d(x, (k, 1), (s, 1), (p, 0), (d, 1), ceil_mode).shape[2]
                            except RuntimeError:
                                assert got <= 0, (size, k, s, p, d, ceil_mode, got)       # torch refuses what the helper calls empty
                                refused += 1
                                continue
                            assert got == want, (size, k, s, p, d, ceil_mode, got, want)
                            n += 1
    assert n > 1000 and refused > 50, (n, refused)         # the sweep reached both: geometries torch takes and ones it refuses


# ---- the module ------------------------------------------------------------------------------------------------------------

def unsigned_pot(threshold=4.0):
    """Unsigned 8 bits, scale threshold / 256, zero point 0: what follows a ReLU."""
    import mct_quantizers_amd as mq
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return mq.pytorch_quantizers.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[threshold], signed=False)


def signed_pot(threshold=4.0):
    """Signed 8 bits, scale threshold / 128, zero point 0, int8 codes."""
    import mct_quantizers_amd as mq
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return mq.pytorch_quantizers.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[threshold], signed=True)


def pot_holder(signed=False):
    import mct_quantizers_amd as mq
    return mq.PytorchActivationQuantizationHolder(signed_pot() if signed else unsigned_pot())


def pot_conv(C, O, k, seed, stride=1):
    """A wrapped convolution without bias whose weights have power-of-two scales (see the module's docstring)."""
    import mct_quantizers_amd as mq
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(C, O, k, stride=stride, padding=k // 2, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn_like(conv.weight) * 0.3 + 0.05)
    return mq.PytorchQuantizationWrapper(conv, {"weight": weights_quantizer(conv.weight, "pot", True)})


def check_module(device):
    """QuantizedMaxPool2d on codes and on float32, against the holder followed by the pool itself; returns the outputs."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    outs = []
    for signed in (False, True):
        holder = pot_holder(signed)
        pool = torch.nn.MaxPool2d(3, 2, 1, ceil_mode=True)
        qpool = consumers.QuantizedMaxPool2d(pool, holder.activation_holder_quantizer)
        scale, zp, qmin, qmax = qpool.activation_code_params()
        assert (scale, zp, qmin, qmax) == ((4.0 / 128, 0, -128, 127) if signed else (4.0 / 256, 0, 0, 255))
        x = (torch.randn(2, 16, 7, 5, generator=torch.Generator().manual_seed(3)) * 2.0).to(device)
        for xx in (x, x.contiguous(memory_format=torch.channels_last)):
            y = qpool(xx)
            assert y.dtype == (torch.int8 if signed else torch.uint8) and y.shape == (2, 16, 4, 3)
            assert y.is_contiguous(memory_format=torch.channels_last)                    # NCHW-shaped, NHWC-stored
            want = pool(holder(xx.cpu()))
            assert torch.equal(ops.dequantize_codes(y.cpu(), scale, zp), want)
            codes = ops.fq_codes_nhwc(xx, qmin, qmax, scale, zp).permute(0, 3, 1, 2)
            assert torch.equal(qpool(codes), y)                                          # codes in: the same codes out
            outs.append(y.cpu())
        with pytest.raises(TypeError):
            qpool(codes.to(torch.uint8 if signed else torch.int8))
        with pytest.raises(TypeError):
            qpool(x.double())
        with pytest.raises(RuntimeError):
            qpool(x[0])
    return outs


def test_quantized_max_pool2d_on_cpu():
    from mct_quantizers_amd import consumers
    check_module("cpu")
    ok = consumers.QuantizedMaxPool2d.eligible
    assert ok(torch.nn.MaxPool2d(2)) and ok(torch.nn.MaxPool2d((3, 2), (2, 3), (1, 0), 2, ceil_mode=True))
    assert not ok(torch.nn.MaxPool2d(2, return_indices=True)) and not ok(torch.nn.MaxPool2d(2, padding=2))
    assert not ok(torch.nn.MaxPool2d((2, 2, 2))) and not ok(torch.nn.MaxPool2d(2.0)) and not ok(torch.nn.MaxPool2d(0))
    assert not ok(torch.nn.AvgPool2d(2)) and not ok(torch.nn.MaxPool1d(2)) and not ok(torch.nn.AdaptiveMaxPool2d(2))

    class Mine(torch.nn.MaxPool2d):                          # exactly nn.MaxPool2d: a subclass may compute anything
        pass

    assert not ok(Mine(2))
    with pytest.raises(TypeError):
        consumers.QuantizedMaxPool2d(torch.nn.MaxPool2d(2, return_indices=True), unsigned_pot())


# ---- the rewrites ----------------------------------------------------------------------------------------------------------

def vgg(device="cpu"):
    """conv -> ReLU -> holder -> MaxPool, twice over, and a last convolution; the layers behind the pools are pointwise."""
    layers = [pot_holder(True), pot_conv(16, 16, 3, 1), torch.nn.ReLU(), pot_holder(), torch.nn.MaxPool2d(2),
              pot_conv(16, 32, 1, 2), torch.nn.ReLU(), pot_holder(), torch.nn.MaxPool2d(2, 2, ceil_mode=True), pot_conv(32, 16, 1, 3)]
    return torch.nn.Sequential(*layers).to(device).eval()


def vgg_input(device="cpu"):
    return (torch.randn(2, 16, 10, 7, generator=torch.Generator().manual_seed(8)) * 1.5).to(device)


class Stem(torch.nn.Module):
    """wrapper (3 channels: no consumer takes it) -> ReLU -> holder -> pool -> two wrapped pointwise convolutions, as the front of
    workloads.wrapped_resnet50.  ``how``: the pool as a module, as ``F.max_pool2d``, or also feeding an add (the negative case)."""

    def __init__(self, how="module"):
        super().__init__()
        self.how = how
        self.c0 = pot_conv(3, 16, 3, 1, stride=2)
        self.act = torch.nn.ReLU()
        self.h = pot_holder()
        self.pool = torch.nn.MaxPool2d(3, 2, 1)
        self.c1, self.down = pot_conv(16, 16, 1, 2), pot_conv(16, 16, 1, 3)

    def forward(self, x):
        a = self.h(self.act(self.c0(x)))
        p = F.max_pool2d(a, 3, stride=2, padding=1) if self.how == "functional" else self.pool(a)
        y = self.c1(p) + self.down(p)
        return y + p if self.how == "add" else y


def stem_input(device="cpu"):
    return (torch.randn(2, 3, 17, 13, generator=torch.Generator().manual_seed(9)) * 1.5).to(device)


def _of(gm, cls):
    return {name: m for name, m in gm.named_modules() if isinstance(m, cls)}


def test_sequential_rewrite_of_a_vgg_style_stack():
    from mct_quantizers_amd import consumers
    C = consumers
    plain, pooled = vgg(), vgg()
    assert C.fuse_linear_consumers(plain, convolutions=True) == 1            # only the first pair: the others sit behind a pool
    assert C.fuse_linear_consumers(pooled, convolutions=True, pools=True) == 3
    kinds = [type(m) for m in pooled]
    assert kinds == [C._FusedAway, C.QuantizedConv2d, torch.nn.ReLU, C._FusedAway, C.QuantizedMaxPool2d, C.QuantizedConv1x1,
                     torch.nn.ReLU, C._FusedAway, C.QuantizedMaxPool2d, C.QuantizedConv1x1]
    assert (pooled[4].kernel_size, pooled[4].stride, pooled[4].ceil_mode) == ((2, 2), (2, 2), False) and pooled[8].ceil_mode
    assert [type(m) for m in plain][3:6] == [type(pot_holder()), torch.nn.MaxPool2d, type(pot_conv(16, 16, 1, 0))]
    x = vgg_input()
    y, y0 = pooled(x), plain(x)
    assert y.shape == (2, 16, 3, 2) and len(torch.unique(y)) > 50 and torch.equal(y, y0)
    assert torch.equal(y, vgg()(x))                      # the products are exact: the untouched model gives the same bits
    # chain=True: a consumer directly in front of the triple emits the pool's codes
    chained = torch.nn.Sequential(pot_holder(True), pot_conv(16, 16, 3, 1), pot_holder(True), torch.nn.MaxPool2d(2), pot_conv(16, 32, 1, 2))
    twin = torch.nn.Sequential(pot_holder(True), pot_conv(16, 16, 3, 1), pot_holder(True), torch.nn.MaxPool2d(2), pot_conv(16, 32, 1, 2))
    assert C.fuse_linear_consumers(chained, convolutions=True, chain=True, pools=True) == 2
    assert C.fuse_linear_consumers(twin, convolutions=True, chain=True) == 1
    assert chained[1].emit_codes_for == chained[3].activation_code_params() == chained[4].activation_code_params()
    seen = []
    hook = chained[3].register_forward_hook(lambda m, args, out: seen.append((args[0].dtype, out.dtype)))
    assert torch.equal(chained(x), twin(x))
    hook.remove()
    assert seen == [(torch.int8, torch.int8)]
    # what the switch leaves alone: a pool with indices, and a Linear behind the pool
    for pool in (torch.nn.MaxPool2d(2, return_indices=True), torch.nn.AvgPool2d(2)):
        m = torch.nn.Sequential(pot_holder(), pool, pot_conv(16, 16, 1, 1))
        assert C.fuse_linear_consumers(m, convolutions=True, pools=True) == 0 and m[1] is pool
    with pytest.raises(TypeError):
        C.fuse_linear_consumers(vgg(), pool=True)


def test_fx_rewrite_of_a_vgg_style_stack():
    from mct_quantizers_amd import consumers
    C = consumers
    x = vgg_input()
    want = vgg()(x)
    # pools alone: a lone holder -> pool loses the holder, the ReLU in front stays
    gm, n = C.fuse_linear_consumers_fx(vgg(), convolutions=True, pools=True)
    gm0, n0 = C.fuse_linear_consumers_fx(vgg(), convolutions=True)
    assert (n, n0) == (3, 1)
    assert _targets(gm) == ["1_qlinear", "2", "4_qpool", "5_qlinear", "6", "8_qpool", "9_qlinear"]
    assert _targets(gm0) == ["1_qlinear", "2", "3", "4", "5", "6", "7", "8", "9"]
    assert torch.equal(gm(x), gm0(x)) and torch.equal(gm(x), want)
    # with shared holders the ReLU is absorbed into a join that writes no float32
    shared = dict(convolutions=True, shared_holders=True)
    gm, n = C.fuse_linear_consumers_fx(vgg(), pools=True, **shared)
    gm0, n0 = C.fuse_linear_consumers_fx(vgg(), **shared)
    assert (n, n0) == (3, 1)
    assert _targets(gm) == ["1_qlinear", "3_join", "4_qpool", "5_qlinear", "7_join", "8_qpool", "9_qlinear"]
    assert all((j.relu, j.has_residual, j.want_float) == (True, False, False) for j in _of(gm, C.QuantizedJoin).values())
    assert not _of(gm0, C.QuantizedJoin) and torch.equal(gm(x), gm0(x))
    # ... and with stay_on_codes the whole stack runs codes to codes: the joins are folded into the producers' clamps
    gm, n = C.fuse_linear_consumers_fx(vgg(), pools=True, stay_on_codes=True, **shared)
    gm0, n0 = C.fuse_linear_consumers_fx(vgg(), stay_on_codes=True, **shared)
    assert (n, n0) == (3, 1)
    assert _targets(gm) == ["1_qlinear", "4_qpool", "5_qlinear", "8_qpool", "9_qlinear"] and not _targets(gm, "call_function")
    assert not _of(gm, C.QuantizedJoin)
    for producer, pool in (("1_qlinear", "4_qpool"), ("5_qlinear", "8_qpool")):
        m = gm.get_submodule(producer)
        assert m.emit_codes_for == gm.get_submodule(pool).activation_code_params() == (4.0 / 256, 0, 0, 255) and m.emit_clamp is None
    assert gm.get_submodule("9_qlinear").emit_codes_for is None
    seen = []
    hooks = [gm.get_submodule(p).register_forward_hook(lambda m, args, out: seen.append((args[0].dtype, out.dtype)))
             for p in ("4_qpool", "8_qpool")]
    y = gm(x)
    for h in hooks:
        h.remove()
    assert seen == [(torch.uint8, torch.uint8)] * 2
    assert torch.equal(y, gm0(x)) and torch.equal(y, want) and len(torch.unique(y)) > 50
    # tracing the rewritten graph again keeps the pool a leaf and replaces nothing more
    again, n = C.fuse_linear_consumers_fx(gm, pools=True, stay_on_codes=True, **shared)
    assert n == 0 and _targets(again) == _targets(gm) and torch.equal(again(x), y)


@pytest.mark.parametrize("how", ["module", "functional"])
def test_fx_rewrite_of_a_resnet_style_stem(how):
    from mct_quantizers_amd import consumers
    import mct_quantizers_amd as mq
    C = consumers
    x = stem_input()
    want = Stem(how)(x)
    pool = "pool_qpool" if how == "module" else "max_pool2d_qpool"
    gm, n = C.fuse_linear_consumers_fx(Stem(how), shared_holders=True, pools=True)
    gm0, n0 = C.fuse_linear_consumers_fx(Stem(how), shared_holders=True)
    assert (n, n0) == (2, 0)
    assert _targets(gm) == ["c0", "h_join", pool, "c1_qlinear", "down_qlinear"]
    assert _targets(gm, "call_function") == [operator.getitem, operator.add] and not _targets(gm, "call_method")
    join = gm.get_submodule("h_join")
    assert (join.relu, join.has_residual, join.want_float) == (True, False, False)
    assert isinstance(gm.get_submodule("c0"), mq.PytorchQuantizationWrapper) and not _of(gm0, C.QuantizedJoin)
    qpool = gm.get_submodule(pool)
    assert (qpool.kernel_size, qpool.stride, qpool.padding, qpool.dilation, qpool.ceil_mode) == ((3, 3), (2, 2), (1, 1), (1, 1), False)
    nodes = {node.target: node for node in gm.graph.nodes if node.op == "call_module"}
    assert nodes["c1_qlinear"].args == nodes["down_qlinear"].args == (nodes[pool],)
    y = gm(x)
    assert y.shape == (2, 16, 5, 4) and len(torch.unique(y)) > 50
    assert torch.equal(y, gm0(x)) and torch.equal(y, want)
    # without shared_holders the holder, whose only user is the pool, goes and the ReLU stays
    gm1, n1 = C.fuse_linear_consumers_fx(Stem(how), pools=True)
    assert n1 == 2 and _targets(gm1) == ["c0", "act", pool, "c1_qlinear", "down_qlinear"] and torch.equal(gm1(x), want)
    # stay_on_codes changes nothing here: the producer is a wrapper
    gm2, n2 = C.fuse_linear_consumers_fx(Stem(how), shared_holders=True, stay_on_codes=True, pools=True)
    assert n2 == 2 and _targets(gm2) == _targets(gm)


def test_fx_rewrite_leaves_a_pool_that_also_feeds_an_add():
    from mct_quantizers_amd import consumers
    for switches in (dict(), dict(shared_holders=True), dict(shared_holders=True, stay_on_codes=True)):
        gm, n = consumers.fuse_linear_consumers_fx(Stem("add"), pools=True, **switches)
        gm0, n0 = consumers.fuse_linear_consumers_fx(Stem("add"), **switches)
        assert n == n0 == 0 and str(gm.graph) == str(gm0.graph) and gm.code == gm0.code
        assert not _of(gm, consumers.QuantizedMaxPool2d) and isinstance(gm.get_submodule("pool"), torch.nn.MaxPool2d)


def test_without_the_keyword_nothing_changes():
    from mct_quantizers_amd import consumers
    for switches in (dict(), dict(convolutions=True), dict(convolutions=True, shared_holders=True),
                     dict(convolutions=True, shared_holders=True, stay_on_codes=True)):
        for make in (vgg, Stem):
            gm, n = consumers.fuse_linear_consumers_fx(make(), **switches)
            gm_off, n_off = consumers.fuse_linear_consumers_fx(make(), pools=False, **switches)
            assert n == n_off and str(gm.graph) == str(gm_off.graph) and gm.code == gm_off.code
            assert not _of(gm, consumers.QuantizedMaxPool2d)


@pytest.mark.parametrize("stay_on_codes", [False, True])
def test_wrapped_resnet50_structure_with_pools(stay_on_codes):
    """Trace and rewrite only.  The stem's max pool now runs on codes, so the first block's c1 and downsample become consumers:
    52 of the 53 convolutions (the 3-channel stem stays a wrapper).  The stem's holder, its ReLU absorbed, becomes one more join,
    which writes no float32: 47 + 1 = 48 joins without ``stay_on_codes``.  With it ``3_a1_1_join``, the ReLU-only join behind the
    first block's c1, is folded as well, c1 now being a consumer that can emit its codes: 16 joins (15 residual ones and the
    stem's) and 32 emitting consumers; the stem's ReLU leaves the ReLU list."""
    from mct_quantizers_amd import consumers, workloads
    switches = dict(convolutions=True, shared_holders=True, stay_on_codes=stay_on_codes)
    gm, n = consumers.fuse_linear_consumers_fx(workloads.wrapped_resnet50(device="cpu"), pools=True, **switches)
    assert n == 52 and len(_of(gm, consumers.IntegerConsumer)) == 52
    pools = _of(gm, consumers.QuantizedMaxPool2d)
    assert list(pools) == ["2_qpool"]
    assert (pools["2_qpool"].kernel_size, pools["2_qpool"].stride, pools["2_qpool"].padding) == ((3, 3), (2, 2), (1, 1))
    called = [gm.get_submodule(t) for t in _targets(gm)]
    assert not [m for m in called if isinstance(m, torch.nn.MaxPool2d)] and torch.nn.functional.max_pool2d not in _targets(gm, "call_function")
    joins = _of(gm, consumers.QuantizedJoin)
    stem = joins["1_1_join"]
    assert (stem.relu, stem.has_residual, stem.want_float) == (True, False, False)
    nodes = {node.target: node for node in gm.graph.nodes if node.op == "call_module"}
    assert sorted(u.target for u in nodes["2_qpool"].users) == ["3_c1_qlinear", "3_down_qlinear"]
    emitting = [m for m in gm.modules() if isinstance(m, consumers.IntegerConsumer) and m.emit_codes_for is not None]
    relus = [t for t in _targets(gm) if isinstance(gm.get_submodule(t), torch.nn.ReLU)]
    assert relus == ["18.a3.0"]                          # the last block's; the stem's went into its join
    if stay_on_codes:
        assert len(joins) == 16 and "3_a1_1_join" not in joins and len(emitting) == 32
        assert sum(j.has_residual for j in joins.values()) == 15
    else:
        assert len(joins) == 48 and "3_a1_1_join" in joins and not emitting


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------

def test_codes_maxpool_argument_validation_needs_no_gpu():
    import os
    import re
    from conftest import REPO
    from mct_quantizers_amd.hip import build, native
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    lib = native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mctq_hip.h")).read(), flags=re.S)
    assert re.search(r"\bmctq_codes_maxpool_nhwc\s*\(", header) and "mctq_codes_maxpool_nhwc" in native.SIGNATURES
    assert lib.mctq_abi_version() == 10 == native.ABI_VERSION
    E, P, I8, U8 = native.MCTQ_E_ARG, 4096, native.CODE_I8, native.CODE_U8      # P: an aligned address that is never dereferenced
    count = lib.mctq_launch_count()
    valid = dict(x=P, y=P, dt=U8, B=2, H=7, W=5, C=16, kh=3, kw=3, sh=2, sw=2, ph=1, pw=1, dh=1, dw=1, ceil=0, ho=4, wo=3)

    def call(**over):
        v = dict(valid, **over)
        return lib.mctq_codes_maxpool_nhwc(v["x"], v["y"], v["dt"], v["B"], v["H"], v["W"], v["C"], v["kh"], v["kw"], v["sh"], v["sw"],
                                           v["ph"], v["pw"], v["dh"], v["dw"], v["ceil"], v["ho"], v["wo"], None)

    def refused(message, **fault):
        assert call(**fault) == E, fault
        assert lib.mctq_last_error() == message, (fault, lib.mctq_last_error())

    for extent in "BHWC":
        refused(b"negative extent", **{extent: -1})
    for name in ("kh", "kw"):
        refused(b"kernel size below 1", **{name: 0})
    for name in ("sh", "sw"):
        refused(b"stride below 1", **{name: 0})
    for name in ("dh", "dw"):
        refused(b"dilation below 1", **{name: 0})
    for name in ("ph", "pw"):
        refused(b"negative padding", **{name: -1})
        refused(b"padding larger than half the kernel size", **{name: 2})
    refused(b"padding larger than half the kernel size", kh=1, ph=1)
    refused(b"channels must be a multiple of 16", C=24)
    for dt in (-1, 2, 3, 77):                                              # the 4-bit code types among them
        refused(b"bad code_dtype", dt=dt)
    refused(b"NULL pointer", x=None)
    refused(b"NULL pointer", y=None)
    refused(b"codes and pooled must be 16-byte aligned", x=P + 8)
    refused(b"codes and pooled must be 16-byte aligned", y=P + 1)
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", kw=3, dw=4, wo=1)             # 9 > 5 + 2
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", H=1, kh=3, ph=0, ho=1)
    # the extent the caller allocated must be the library's own: one more or one less, either axis, and the ceil_mode rule
    for name, value in (("ho", 3), ("ho", 5), ("wo", 2), ("wo", 4), ("ho", 0), ("wo", -1)):
        refused(b"out_height / out_width are not the pooled extent", **{name: value})
    assert call(kh=2, kw=2, ph=1, pw=1, ceil=1, ho=4, wo=3, B=0) == 0                                       # both last windows dropped
    refused(b"out_height / out_width are not the pooled extent", kh=2, kw=2, ph=1, pw=1, ceil=1, ho=5, wo=3)
    refused(b"out_height / out_width are not the pooled extent", kh=2, kw=2, ph=1, pw=1, ceil=1, ho=4, wo=4)
    refused(b"out_height / out_width are not the pooled extent", kh=2, kw=2, ph=0, pw=0, ceil=0, ho=4, wo=3)   # 3 x 2 without ceil_mode
    assert call(kh=2, kw=2, ph=0, pw=0, ceil=1, ho=4, wo=3, B=0) == 0
    refused(b"too many output pixels for one launch", B=2 ** 31, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0, H=1, W=1, ho=1, wo=1)
    refused(b"more than 2^32 - 1 16-channel chunks of output in one launch", B=2 ** 30, C=64, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0,
            H=1, W=1, ho=1, wo=1)
    refused(b"padded image extent exceeds 2^31 - 1", H=2 ** 31, ho=2 ** 30)
    refused(b"padded image extent exceeds 2^31 - 1", H=2 ** 31 - 4, W=0)              # H + 2 + 3 with the kernel's span; W: no fit
    refused(b"an image of a non-empty batch needs at least one pixel", H=0, kh=2, ph=1, sh=1, ho=1)
    # wrong in two ways: the window's sizes, the half-kernel rule, the channels, the code type, the fit, the extent, the pixels
    refused(b"negative padding", ph=-1, pw=2)
    refused(b"padding larger than half the kernel size", pw=2, C=24)
    refused(b"channels must be a multiple of 16", C=24, dt=77)
    refused(b"bad code_dtype", dt=77, kw=3, dw=4)
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", kw=3, dw=4, wo=7)
    refused(b"out_height / out_width are not the pooled extent", H=0, kh=2, ph=1, sh=1, ho=2, x=None)
    assert call(B=0) == 0 and call(B=0, x=None, y=None) == 0          # no images: no launch, no pointer is looked at
    assert call(C=0) == 0                                               # no channels: nothing to write
    assert call(B=0, dt=I8) == 0
    assert lib.mctq_launch_count() == count                            # refused and empty calls launch nothing
