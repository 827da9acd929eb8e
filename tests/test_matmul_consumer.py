"""consumers.qmatmul_i8 / QuantizedMatmul / fuse_linear_consumers_fx(matmuls=True) on the CPU route, which is the contract:

    acc[m][n] = sum_k (a[m][k] - za) * (b[k][n] - zb)      exact
    y = float32(acc) * (float32(sa) * float32(sb))          one rounding per operation
    codes = clamp(rint(y * (1 / so)) + zo, lo, hi)

checked against a brute-force int64 einsum in numpy, at the edges of the code types and of K, and through the graph rewrite of
workloads.wrapped_attention_block.  tests/test_gpu_matmul_consumer.py holds the kernel to this route bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import bits_equal, first_mismatch

PAIRS = [(False, False), (True, False), (False, True), (True, True)]             # (a is uint8, b is uint8)
ZERO_POINTS = {True: (0, 255, 131), False: (0, -128, 127, -3)}                   # 0, both ends of the code type, one inside
OUT_FORMS = {True: (0.37, 114, 0, 255), False: (0.41, -5, -128, 127)}

ALL_SWITCHES = dict(chain=True, uniform_weights=True, convolutions=True, depthwise=True, shared_holders=True, stay_on_codes=True,
                    pools=True, fused_residuals=True, concats=True, avg_pools=True, muls=True, hard_activations=True,
                    upsamples=True, any_channels=True, activation_tables=True, grouped=True, transposed=True)


def rand_codes(shape, u8, rng):
    lo, hi = (0, 256) if u8 else (-128, 128)
    return torch.from_numpy(rng.integers(lo, hi, size=shape).astype(np.uint8 if u8 else np.int8))


def brute_acc(a, za, b, zb, transposed_b):
    """The int64 sums by einsum, batch dimensions broadcast: a [..., M, K], b [..., N, K] (transposed_b) or [..., K, N]."""
    a64, b64 = a.numpy().astype(np.int64) - za, b.numpy().astype(np.int64) - zb
    return np.einsum("...mk,...nk->...mn" if transposed_b else "...mk,...kn->...mn", a64, b64)


def contract(acc, sa, sb, out_codes=None):
    """float32(acc) * (float32(sa) * float32(sb)), and the codes of ``out_codes`` = (scale, zp, qmin, qmax) of it, in numpy."""
    f32 = np.float32
    y = acc.astype(f32) * (f32(sa) * f32(sb))
    if out_codes is None:
        return y
    so, zo, qmin = out_codes[:3]
    lo, hi = out_codes[-2:]                                                # the domain's ends, or a folded clamp inside it
    q = np.clip(np.rint(y * (f32(1.0) / f32(so))) + f32(zo), lo, hi)
    return q.astype(np.uint8 if qmin >= 0 else np.int8)


def check_against_brute(a, fa, b, fb, transposed_b, out_codes, what=None):
    from mct_quantizers_amd import consumers
    got = consumers.qmatmul_i8(a, fa, b, fb, transposed_b=transposed_b, out_codes=out_codes)
    want = contract(brute_acc(a.cpu(), fa[1], b.cpu(), fb[1], transposed_b), fa[0], fb[0], out_codes)
    if out_codes is None:
        assert got.dtype == torch.float32 and bits_equal(got.cpu().numpy(), want), (what, first_mismatch(got.cpu().numpy(), want))
    else:
        assert got.dtype == (torch.uint8 if out_codes[2] >= 0 else torch.int8)
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want), what
    return got


# (a's batch, b's batch, M, N, K): 2-D operands; equal batches; broadcast batch dimensions with M = 1 and K = 1; a 3-D with a 2-D
SHAPES = [((), (), 5, 7, 19), ((2, 3), (2, 3), 5, 7, 19), ((2, 1), (3,), 1, 4, 1), ((4,), (), 3, 16, 33), ((1, 2), (5, 1), 2, 3, 64)]


@pytest.mark.parametrize("transposed_b", [True, False])
@pytest.mark.parametrize("a_u8,b_u8", PAIRS)
def test_cpu_route_equals_the_int64_einsum(a_u8, b_u8, transposed_b):
    rng = np.random.default_rng(7 + 2 * a_u8 + b_u8)
    n = 0
    for ba, bb, M, N, K in SHAPES:
        for za in ZERO_POINTS[a_u8]:
            for zb in ZERO_POINTS[b_u8][:3]:
                a = rand_codes((*ba, M, K), a_u8, rng)
                b = rand_codes((*bb, N, K) if transposed_b else (*bb, K, N), b_u8, rng)
                out_codes = (None, OUT_FORMS[True], OUT_FORMS[False])[n % 3]
                if out_codes is not None:                                  # a scale that spreads the sums over the codes
                    out_codes = (0.9 * 0.7 * 128 * 64 * np.sqrt(K) / 100, *out_codes[1:])
                y = check_against_brute(a, (0.9, za), b, (0.7, zb), transposed_b, out_codes, (ba, bb, M, N, K, za, zb))
                assert y.shape == (*np.broadcast_shapes(ba, bb), M, N)
                n += 1
    assert n == len(SHAPES) * len(ZERO_POINTS[a_u8]) * 3


def test_one_dimensional_operands_are_taken_as_torch_matmul_takes_them():
    from mct_quantizers_amd import consumers
    rng = np.random.default_rng(3)
    a, b, v = rand_codes((2, 5, 19), True, rng), rand_codes((19, 4), False, rng), rand_codes((19,), False, rng)
    fa, fb = (0.5, 7), (0.25, -2)
    for x0, f0, x1, f1 in ((a, fa, v, fb), (v, fb, b, fb), (v, fb, v, fb)):
        got = consumers.qmatmul_i8(x0, f0, x1, f1, transposed_b=False)
        want = torch.matmul(x0.double() - f0[1], x1.double() - f1[1]).float() * (f0[0] * f1[0])
        assert got.shape == want.shape and torch.equal(got, want)
    # the transpose of a vector is the vector
    assert torch.equal(consumers.qmatmul_i8(a, fa, v, fb, transposed_b=True), consumers.qmatmul_i8(a, fa, v, fb, transposed_b=False))


@pytest.mark.parametrize("a_u8,b_u8", PAIRS)
def test_all_65536_code_pairs(a_u8, b_u8):
    """[256, 1] x [1, 256]: every pair of codes once, K = 1, zero points inside both types."""
    col = lambda u8: torch.arange(256, dtype=torch.uint8) if u8 else torch.arange(-128, 128).to(torch.int8)   # noqa: E731
    a, za, zb = col(a_u8).reshape(256, 1), (77 if a_u8 else -9), (201 if b_u8 else 55)
    for transposed_b in (True, False):
        b = col(b_u8).reshape(256, 1) if transposed_b else col(b_u8).reshape(1, 256)
        y = check_against_brute(a, (0.5, za), b, (0.125, zb), transposed_b, None)
        want = (a.double() - za) * (col(b_u8).double().reshape(1, 256) - zb) * 0.0625
        assert torch.equal(y.double(), want)                               # 0.0625 * an integer below 2^16: exact
        check_against_brute(a, (0.5, za), b, (0.125, zb), transposed_b, (16.0, 3, -128, 127))
        check_against_brute(a, (0.5, za), b, (0.125, zb), transposed_b, (20.0, 100, 0, 255, 10, 200))    # a folded clamp


@pytest.mark.parametrize("transposed_b", [True, False])
@pytest.mark.parametrize("a_u8,b_u8", PAIRS)
def test_the_largest_sums_come_out_exactly(a_u8, b_u8, transposed_b):
    """K = 32768 with every code at the extreme that maximises |acc| = 255 * 255 * 32768 = 2130739200 < 2^31, both signs."""
    K = 32768
    ends = lambda u8: ((0, 255) if u8 else (-128, 127))                   # noqa: E731
    (alo, ahi), (blo, bhi) = ends(a_u8), ends(b_u8)
    dt = lambda u8: torch.uint8 if u8 else torch.int8                      # noqa: E731
    a = torch.full((2, K), ahi, dtype=dt(a_u8))                            # za = alo: a - za = 255
    b = torch.full((2, K), bhi, dtype=dt(b_u8))
    b[1] = blo                                                             # column 0: zb = blo -> +255; column 1 read with zb = bhi -> -255
    for zb, want in ((blo, [[2130739200, 0]] * 2), (bhi, [[0, -2130739200]] * 2)):
        bb = b if transposed_b else b.t().contiguous()
        assert brute_acc(a, alo, bb, zb, transposed_b).tolist() == want
        y = check_against_brute(a, (1.0, alo), bb, (1.0, zb), transposed_b, None)
        assert y.tolist() == [[float(np.float32(v)) for v in row] for row in want]
        # codes: one step per 2^24 of the sum -- 127 steps, the last partly
        codes = check_against_brute(a, (1.0, alo), bb, (1.0, zb), transposed_b, (float(2 ** 24), 0, -128, 127))
        assert codes.tolist() == [[round(v / 2 ** 24) for v in row] for row in want]


def _holders(pot=True):
    import mct_quantizers_amd as mq
    Q = mq.pytorch_quantizers
    qa = Q.ActivationSymmetricInferableQuantizer(8, [4.0], True)
    qb = Q.ActivationSymmetricInferableQuantizer(8, [2.0], False)
    qc = Q.ActivationSymmetricInferableQuantizer(8, [64.0], True)
    return [(q, mq.PytorchActivationQuantizationHolder(q)) for q in (qa, qb, qc)]


@pytest.mark.parametrize("transposed_b", [True, False])
def test_module_equals_the_float_chain_where_that_is_exact(transposed_b):
    """Power-of-two scales and K = 64: 255 * 255 * 64 < 2^24, so torch.matmul of the two holder outputs is exact."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    (qa, ha), (qb, hb), (qc, hc) = _holders()
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 9, 64, generator=gen) * 2
    y = torch.rand(2, 3, 11, 64, generator=gen) * 2.2
    if not transposed_b:
        y = y.transpose(-1, -2).contiguous()
    want = torch.matmul(ha(x), hb(y).transpose(-1, -2) if transposed_b else hb(y))
    m = consumers.QuantizedMatmul([qa, qb], transposed_b=transposed_b)
    assert m.activation_code_params() is None and m.operand_code_params(1) == (2.0 / 256, 0, 0, 255)
    assert torch.equal(m(x, y), want)
    # operands as codes, as float32, mixed: the same result
    ca = ops.fq_codes(x, None, None, None, -128, 127, 4.0 / 128, 0)
    cb = ops.fq_codes(y, None, None, None, 0, 255, 2.0 / 256, 0)
    assert torch.equal(m(ca, cb), want) and torch.equal(m(ca, y), want) and torch.equal(m(ha(x), cb), want)
    # as codes behind a holder
    mc = consumers.QuantizedMatmul([qa, qb], qc, transposed_b=transposed_b)
    codes = mc(x, y)
    assert codes.dtype == torch.int8 and mc.activation_code_params() == (0.5, 0, -128, 127)
    assert torch.equal(ops.dequantize_codes(codes, 0.5, 0), hc(want)) and len(codes.unique()) > 20


def test_argument_errors():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    Q = mq.pytorch_quantizers
    a, b = torch.zeros(2, 3, 16, dtype=torch.uint8), torch.zeros(2, 5, 16, dtype=torch.int8)
    ok = lambda **kw: consumers.qmatmul_i8(kw.get("a", a), kw.get("fa", (0.5, 3)), kw.get("b", b), kw.get("fb", (0.5, -3)),   # noqa: E731
                                           transposed_b=kw.get("t", True), out_codes=kw.get("out"))
    assert ok().shape == (2, 3, 5)
    with pytest.raises(TypeError, match="int8 / uint8 codes"):
        ok(a=a.float())
    with pytest.raises(TypeError, match="int8 / uint8 codes"):
        ok(b=b.to(torch.int32))
    with pytest.raises(ValueError, match="is no torch.uint8 code"):
        ok(fa=(0.5, -1))
    with pytest.raises(ValueError, match="is no torch.int8 code"):
        ok(fb=(0.5, 128))
    with pytest.raises(ValueError, match="finite and positive"):
        ok(fa=(0.0, 3))
    with pytest.raises(ValueError, match="finite and positive"):
        ok(fb=(float("inf"), 3))
    with pytest.raises(RuntimeError, match="K=16.*K=5"):
        ok(t=False)                                                        # b read as [K = 5, N = 16]
    with pytest.raises(NotImplementedError, match="K <= 32768"):
        ok(a=torch.zeros(1, 32769, dtype=torch.uint8), b=torch.zeros(1, 32769, dtype=torch.int8))
    with pytest.raises(NotImplementedError, match="K <= 32768"):
        ok(a=torch.zeros(3, 0, dtype=torch.uint8), b=torch.zeros(5, 0, dtype=torch.int8))
    with pytest.raises(ValueError, match="narrowed clamp"):
        ok(out=(0.5, 0, 0, 255, -1, 300))
    with pytest.raises(ValueError, match="does not fit an 8-bit code"):
        ok(out=(0.5, 0, -300, 300))
    # the module: the same exception classes as QuantizedMul / QuantizedConcat
    q8 = Q.ActivationSymmetricInferableQuantizer(8, [4.0], True)
    with pytest.raises(NotImplementedError, match="wider than 8 bits"):
        consumers.QuantizedMatmul([q8, Q.ActivationSymmetricInferableQuantizer(9, [4.0], True)])
    with pytest.raises(NotImplementedError, match="wider than 8 bits"):
        consumers.QuantizedMatmul([q8, q8], Q.ActivationSymmetricInferableQuantizer(16, [4.0], True))
    with pytest.raises(TypeError, match="per-tensor"):
        consumers.QuantizedMatmul([q8, Q.WeightsSymmetricInferableQuantizer(8, [1.0, 2.0], True, 0)])
    with pytest.raises(ValueError, match="two operands"):
        consumers.QuantizedMatmul([q8])
    m = consumers.QuantizedMatmul([q8, q8])
    with pytest.raises(TypeError, match="do not match"):
        m(torch.zeros(2, 16, dtype=torch.uint8), torch.zeros(16, 2))      # uint8 codes for a signed quantizer
    with pytest.raises(TypeError, match="float32 tensors or activation codes"):
        m(torch.zeros(2, 16, dtype=torch.float16), torch.zeros(16, 2))
    # QuantizedMul / QuantizedConcat still need their output quantizer
    with pytest.raises(NotImplementedError):
        consumers.QuantizedMul([q8, q8], None)


def test_native_argument_validation_needs_no_gpu():
    from mct_quantizers_amd.hip import native
    lib = native.load()
    A, B, Y = 0x10000, 0x20000, 0x30000                                    # never read: every call below returns before a launch

    def call(a=A, b=B, y=Y, adt=native.CODE_U8, za=3, sa=0.5, astr=(1024, 512, 32), bdt=native.CODE_I8, zb=-3, sb=0.5,
             bstr=(1024, 512, 32), t=1, form=(-1, 1.0, 0, 0, 0), dims=(2, 2, 16, 16, 32)):
        return lib.mctq_qmatmul_i8(a, adt, za, sa, *astr, b, bdt, zb, sb, *bstr, t, y, *form, *dims, None)

    def refused(words, **kw):
        assert call(**kw) == native.MCTQ_E_ARG
        assert words in lib.mctq_last_error().decode(), lib.mctq_last_error()

    refused("bad a_code_dtype", adt=7)
    refused("bad b_code_dtype", bdt=-1)
    refused("a_zero_point is no code of a_code_dtype", za=256)
    refused("b_zero_point is no code of b_code_dtype", zb=-129)
    refused("a_scale must be finite and positive", sa=0.0)
    refused("b_scale must be finite and positive", sb=float("nan"))
    refused("negative extent", dims=(2, 2, -1, 16, 32))
    refused("K outside 1 .. 32768", dims=(2, 2, 16, 16, 0))
    refused("K outside 1 .. 32768", dims=(2, 2, 16, 16, 32769))
    refused("bad y_code_dtype", form=(9, 1.0, 0, 0, 255))
    refused("clamp domain does not fit the code type", form=(native.CODE_I8, 1.0, 0, 0, 255))
    refused("N must be a multiple of 16", t=0, dims=(2, 2, 16, 24, 32))
    refused("batch0 * batch1 > 65535", dims=(256, 256, 16, 16, 32))
    refused("a_codes: the batch and row strides must be multiples of 16 bytes", astr=(1024, 512, 40))
    refused("b_codes: the batch and row strides must be multiples of 16 bytes", bstr=(1000, 512, 32))
    refused("a_codes: negative stride", astr=(-1024, 512, 32))
    refused("a_codes: the row stride is shorter than a row", astr=(1024, 512, 16))
    refused("b_codes: the row stride is shorter than a row", t=0, bstr=(1024, 512, 16), dims=(2, 2, 16, 32, 32))     # [K, N = 32]
    refused("NULL pointer", a=None)
    refused("16-byte aligned", b=B + 8)
    refused("the output overlaps an operand", y=A + 1024)                 # inside a's 2 x 2 x 16 rows
    refused("the output overlaps an operand", y=B - 16)                   # float32 [2, 2, 16, 16] reaches into b
    # an empty product returns 0 without a launch, whatever the pointers
    for dims in ((0, 2, 16, 16, 32), (2, 0, 16, 16, 32), (2, 2, 0, 16, 32), (2, 2, 16, 0, 32)):
        assert call(a=None, b=None, y=None, dims=dims) == 0


# ---- the graph rewrite ---------------------------------------------------------------------------------------------------

def _nodes(gm):
    return [(n.op, n.target if isinstance(n.target, str) else n.target.__name__) for n in gm.graph.nodes]


def _block(**kw):
    from mct_quantizers_amd import workloads
    return workloads.wrapped_attention_block(**kw)


BLOCK_INPUT = torch.randn(3, 17, 64, generator=torch.Generator().manual_seed(11)) * 1.5

# what fuse_linear_consumers_fx made of the block before ``matmuls`` existed, with every switch and with none
PARENT_NODES_ALL = [
    ('placeholder', 'x'), ('call_module', 'norm'), ('call_module', 'a_in_join'), ('call_function', 'getitem'),
    ('call_module', 'q_qlinear'), ('call_module', 'a_q'), ('call_method', 'reshape'), ('call_method', 'permute'),
    ('call_module', 'k_qlinear'), ('call_module', 'a_k'), ('call_method', 'reshape'), ('call_method', 'permute'),
    ('call_module', 'v_qlinear'), ('call_module', 'a_v'), ('call_method', 'reshape'), ('call_method', 'permute'),
    ('call_method', 'transpose'), ('call_function', 'matmul'), ('call_module', 'a_scores'), ('call_function', 'mul'),
    ('call_module', 'a_scaled'), ('call_method', 'softmax'), ('call_module', 'a_probs'), ('call_function', 'matmul'),
    ('call_module', 'a_ctx'), ('call_method', 'permute'), ('call_method', 'reshape'), ('call_module', 'proj'), ('output', 'output')]
PARENT_NODES_NONE = [(op, {"a_in_join": "a_in", "q_qlinear": "q", "k_qlinear": "k", "v_qlinear": "v"}.get(t, t))
                     for op, t in PARENT_NODES_ALL if (op, t) != ('call_function', 'getitem')]


def test_without_the_switch_the_graph_is_what_it_was():
    from mct_quantizers_amd import consumers
    for switches, nodes, count in ((ALL_SWITCHES, PARENT_NODES_ALL, 3), ({}, PARENT_NODES_NONE, 0)):
        gm, n = consumers.fuse_linear_consumers_fx(_block(), **switches)
        gm_off, n_off = consumers.fuse_linear_consumers_fx(_block(), matmuls=False, **switches)
        assert n == n_off == count and _nodes(gm) == _nodes(gm_off) == nodes
        assert not any(isinstance(m, consumers.QuantizedMatmul) for m in gm.modules())
        assert torch.equal(gm(BLOCK_INPUT), _block()(BLOCK_INPUT))         # POT scales, dim = 64: every product is exact


@pytest.mark.parametrize("switches", [ALL_SWITCHES, {}], ids=["every switch", "matmuls alone"])
def test_rewrite_of_the_attention_block(switches):
    from mct_quantizers_amd import consumers
    stay = bool(switches)
    gm, n = consumers.fuse_linear_consumers_fx(_block(), matmuls=True, **switches)
    base, n_base = consumers.fuse_linear_consumers_fx(_block(), **switches)
    assert n == n_base + 1                                                 # the projection behind the context, now a consumer
    nodes = _nodes(gm)
    front = [('placeholder', 'x'), ('call_module', 'norm'), ('call_module', 'a_in_join'), ('call_function', 'getitem')] if stay \
        else [('placeholder', 'x'), ('call_module', 'norm'), ('call_module', 'a_in')]
    qkv = [(('call_module', name + ("_qlinear" if stay else "")), ('call_method', 'reshape'), ('call_method', 'permute')) for name in "qkv"]
    assert nodes == front + [x for triple in qkv for x in triple] + [
        ('call_module', 'matmul_qmatmul'), ('call_module', 'a_scores'), ('call_function', 'mul'), ('call_module', 'a_scaled'),
        ('call_method', 'softmax'), ('call_module', 'matmul_1_qmatmul'), ('call_method', 'permute'), ('call_method', 'reshape'),
        ('call_module', 'proj_qlinear'), ('output', 'output')]
    # both products are QuantizedMatmul; the transpose went into the first and is not executed
    scores, context = gm.get_submodule("matmul_qmatmul"), gm.get_submodule("matmul_1_qmatmul")
    assert type(scores) is type(context) is consumers.QuantizedMatmul
    assert scores.transposed_b and not context.transposed_b and ('call_method', 'transpose') not in nodes
    # the scores leave in float32 (the scale multiply and the softmax are float32); the context leaves as a_ctx's codes
    assert scores.activation_code_params() is None
    assert context.activation_code_params() == (2.0 / 128, 0, -128, 127) == gm.get_submodule("proj_qlinear").activation_code_params()
    assert context.operand_code_params(0) == (1.0 / 256, 0, 0, 255)        # the probabilities' holder went into the module
    if stay:                                                               # q, k, v leave their consumers as codes
        for name, (m, i) in (("q", (scores, 0)), ("k", (scores, 1)), ("v", (context, 1))):
            assert gm.get_submodule(name + "_qlinear").emit_codes_for == m.operand_code_params(i) == (4.0 / 128, 0, -128, 127)
    else:
        assert type(gm.get_submodule("q")).__name__ == "PytorchQuantizationWrapper"
    y = gm(BLOCK_INPUT)
    assert y.dtype == torch.float32 and y.shape == (3, 17, 64)
    assert torch.equal(y, base(BLOCK_INPUT)) and torch.equal(y, _block()(BLOCK_INPUT))
    assert len(y.unique()) > 100


def test_codes_flow_between_the_consumers_and_the_products():
    """With stay_on_codes the tensors between q / k / v and the products, and between the context and the projection, are int8."""
    from mct_quantizers_amd import consumers
    gm, _ = consumers.fuse_linear_consumers_fx(_block(), matmuls=True, **ALL_SWITCHES)
    seen = {}
    for name in ("q_qlinear", "k_qlinear", "v_qlinear", "matmul_qmatmul", "matmul_1_qmatmul"):
        gm.get_submodule(name).register_forward_hook(lambda m, args, out, name=name: seen.__setitem__(name, (tuple(a.dtype for a in args), out.dtype)))
    gm(BLOCK_INPUT)
    assert seen["q_qlinear"][1] == seen["k_qlinear"][1] == seen["v_qlinear"][1] == torch.int8
    assert seen["matmul_qmatmul"] == ((torch.int8, torch.int8), torch.float32)
    assert seen["matmul_1_qmatmul"] == ((torch.float32, torch.int8), torch.int8)


@pytest.mark.parametrize("switches", [ALL_SWITCHES, {}], ids=["every switch", "matmuls alone"])
def test_rewrite_of_the_fused_qkv_variant(switches):
    """timm's form: one qkv Linear and holder, reshape, permute(2, 0, 3, 1, 4) and three getitem nodes -- the permute has three
    users, all of which lead to operands of the two products."""
    from mct_quantizers_amd import consumers
    gm, n = consumers.fuse_linear_consumers_fx(_block(fused_qkv=True), matmuls=True, **switches)
    assert n == 2 and _nodes(gm) == [
        ('placeholder', 'x'), ('call_module', 'norm'), ('call_module', 'qkv_qlinear'), ('call_method', 'reshape'),
        ('call_method', 'permute'), ('call_function', 'getitem'), ('call_function', 'getitem'), ('call_function', 'getitem'),
        ('call_module', 'matmul_qmatmul'), ('call_module', 'a_scores'), ('call_function', 'mul'), ('call_module', 'a_scaled'),
        ('call_method', 'softmax'), ('call_module', 'matmul_1_qmatmul'), ('call_method', 'permute'), ('call_method', 'reshape'),
        ('call_module', 'proj_qlinear'), ('output', 'output')]
    scores = gm.get_submodule("matmul_qmatmul")
    assert scores.transposed_b and gm.get_submodule("matmul_1_qmatmul").activation_code_params() is not None
    assert gm.get_submodule("qkv_qlinear").emit_codes_for == (scores.operand_code_params(0) if switches else None)
    want = _block(fused_qkv=True)(BLOCK_INPUT)
    assert torch.equal(gm(BLOCK_INPUT), want) and len(want.unique()) > 100


def test_uniform_holders_differ_from_the_float_chain_by_its_rounding_only():
    """Zero points that are not 0 and scales that are no powers of two: the rewrite is the exact sum scaled once, the float32 chain
    accumulates in float32; the block's outputs agree to a few steps of the last holder."""
    from mct_quantizers_amd import consumers
    gm, _ = consumers.fuse_linear_consumers_fx(_block(uniform=True), matmuls=True, **ALL_SWITCHES)
    scores = gm.get_submodule("matmul_qmatmul")
    assert scores.operand_code_params(0)[1] != 0 and scores.operand_code_params(1)[1] != 0
    y, want = gm(BLOCK_INPUT), _block(uniform=True)(BLOCK_INPUT)
    assert (y - want).abs().max() < 0.1 and (y - want).abs().mean() < 1e-3


class _SideUser(nn.Module):
    """Two holders in front of a product; the first also has a float32 user."""

    def __init__(self, spelling):
        super().__init__()
        (_, self.ha), (_, self.hb), (_, self.hc) = _holders()
        self.spelling = spelling

    def forward(self, x, y):
        a, b = self.ha(x), self.hb(y)
        if self.spelling == "matmul":
            p = torch.matmul(a, b.transpose(-2, -1))
        elif self.spelling == "method":
            p = a.matmul(b.reshape(-1, 11, 64).transpose(1, 2))            # positive indices: the reshape tells the rank
        elif self.spelling == "permute":
            p = a @ b.permute(0, 2, 1)                                     # no transpose node: the NN form on a strided view
        else:
            p = torch.bmm(a, b.mT)
        return self.hc(p), a.sum()


@pytest.mark.parametrize("spelling", ["matmul", "method", "permute", "bmm"])
def test_a_holder_with_a_float32_side_user_stays(spelling):
    from mct_quantizers_amd import consumers
    model = _SideUser(spelling)
    gm, n = consumers.fuse_linear_consumers_fx(model, matmuls=True)
    nodes = _nodes(gm)
    assert n == 0 and ('call_module', 'ha') in nodes and ('call_module', 'hb') not in nodes     # hb went into the module
    assert ('call_module', 'hc') in nodes                                  # its user is the output: float32, so it stays
    [mm] = [m for m in gm.modules() if isinstance(m, consumers.QuantizedMatmul)]
    assert mm.activation_code_params() is None
    assert mm.transposed_b == (spelling != "permute")
    assert not any(t in ("transpose", "getattr") for _, t in nodes)       # an absorbed transpose is not executed
    gen = torch.Generator().manual_seed(2)
    x, y = torch.randn(3, 9, 64, generator=gen), torch.rand(3, 11, 64, generator=gen) * 2
    (p, s), (wp, ws) = gm(x, y), model(x, y)
    assert torch.equal(p, wp) and torch.equal(s, ws)


def test_operands_that_reach_no_holder_and_other_products_are_left_alone():
    from mct_quantizers_amd import consumers

    class NoHolder(nn.Module):
        def __init__(self):
            super().__init__()
            (_, self.ha), (_, self.hb), _ = _holders()

        def forward(self, x, y):
            a = self.ha(x)
            return a @ y.transpose(-1, -2), a @ torch.relu(self.hb(y)).transpose(-1, -2), torch.einsum("bmk,bnk->bmn", a, self.hb(y)), \
                torch.matmul(a, self.hb(y).view(torch.float32).mT)

    gm, n = consumers.fuse_linear_consumers_fx(NoHolder(), matmuls=True)
    assert n == 0 and not any(isinstance(m, consumers.QuantizedMatmul) for m in gm.modules())


class _SharedAndGated(nn.Module):
    """Holder ``ha`` feeds a wrapped Linear and, through a reshape, a product (a join hands both its codes with
    ``shared_holders``); the product's holder ``hc`` feeds a multiply with a gate, whose holder feeds a wrapped Linear."""

    def __init__(self):
        super().__init__()
        import mct_quantizers_amd as mq
        Q = mq.pytorch_quantizers
        (_, self.ha), (_, self.hb), (_, self.hc) = _holders()
        hold = lambda thr, signed: mq.PytorchActivationQuantizationHolder(Q.ActivationSymmetricInferableQuantizer(8, [thr], signed))   # noqa: E731
        self.hg, self.hm = hold(1.0, False), hold(64.0, True)
        gen = torch.Generator().manual_seed(3)

        def wrap(cin, cout):
            layer = nn.Linear(cin, cout, bias=False)
            with torch.no_grad():
                layer.weight.copy_(torch.randn(cout, cin, generator=gen) * 0.25)
            return mq.PytorchQuantizationWrapper(layer, {"weight": Q.WeightsPOTInferableQuantizer(8, [1.0] * cout, True, 0)})

        self.side, self.last = wrap(64, 16), wrap(16, 16)

    def forward(self, x, y, g):
        a = self.ha(x)
        p = self.hc(a.reshape(-1, 9, 64) @ self.hb(y).mT)                  # [B, 9, 16]
        return self.last(self.hm(p * self.hg(g))), self.side(a)


def test_a_join_hands_its_codes_to_the_product_and_a_multiply_reads_the_products_codes():
    from mct_quantizers_amd import consumers
    gen = torch.Generator().manual_seed(4)
    x, y, g = torch.randn(2, 9, 64, generator=gen), torch.rand(2, 16, 64, generator=gen) * 2, torch.rand(2, 9, 16, generator=gen)
    want = _SharedAndGated()(x, y, g)
    gm, n = consumers.fuse_linear_consumers_fx(_SharedAndGated(), matmuls=True, muls=True, shared_holders=True, stay_on_codes=True)
    nodes = _nodes(gm)
    assert n == 2 and ('call_module', 'ha_join') in nodes and ('call_module', 'ha') not in nodes
    assert not any(t in ("hb", "hc", "hg", "hm") for _, t in nodes)        # all absorbed: the product and the multiply quantize
    [mm] = [m for m in gm.modules() if isinstance(m, consumers.QuantizedMatmul)]
    mul = gm.get_submodule("hm_mul")
    assert mm.transposed_b and mm.activation_code_params() == mul.operand_code_params(0) == (0.5, 0, -128, 127)
    seen = {}
    for name, m in gm.named_modules():
        if isinstance(m, (consumers.QuantizedMatmul, consumers.QuantizedMul, consumers.QuantizedJoin)):
            m.register_forward_hook(lambda m, args, out, name=name: seen.__setitem__(name, [a.dtype for a in args]))
    got = gm(x, y, g)
    assert seen["ha_join"] == [torch.float32] and seen["hm_mul"][0] == torch.int8
    assert [d for k, d in seen.items() if "qmatmul" in k] == [[torch.int8, torch.float32]]      # the join's codes; y quantized inside
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
