"""mctq_codes_table, consumers.QuantizedActivationTable and the ``activation_tables`` rewrite on the GPU.

The raw entry point must equal the CPU route of ops.codes_table byte for byte, for every byte value at every position of a
16-byte chunk, at every element count at which the kernel takes another path (the byte tail alone, whole chunks, a partly empty
last workgroup, several workgroups), for every value of the tuning key "table_chunks", and write nothing outside its output.

On the GPU ATen's elementwise kernels apply one scalar functor per element whatever its position, so the module's codes are
those of the float32 chain A -> f -> B on the device for EVERY accepted function, the transcendental ones included: strict
equality here, where the CPU tests (tests/test_table_consumer.py) have to exclude the elements ATen's vector body and scalar tail
round differently.  A function that fails here leaves the accepted list."""
import numpy as np
import pytest
import torch

from test_table_consumer import (ACCEPTED, ALL, HOLDER_PAIRS, SHAPES, DecoderStage, MBConv, TwoNodes, check_refusals, float_chain, input_of,
                                 model_args, permutation_table, rewritten, table_module)

GUARD, SENTINEL = 64, 0xA5
CHUNKS = (1, 2, 4)                                           # the values of the tuning key "table_chunks"; 4 is the default


def covered(chunks):
    """S: the bytes one workgroup covers -- 256 lanes, ``chunks`` chunks of 16 bytes each."""
    return 256 * chunks * 16


def blocks_for(n, chunks):
    """The workgroups of a launch over n bytes: whole chunks in groups of S / 16; the n % 16 tail rides with the first."""
    return max(1, -(-(n // 16) // (covered(chunks) // 16)))


def every_byte_everywhere(n):
    """n bytes in which every byte value stands at every position of a 16-byte chunk (once n reaches 16 * 256): byte i holds
    (i // 16 + 37 * (i % 16)) mod 256, scrambled between the 4 KiB periods so that the workgroups differ."""
    i = np.arange(n, dtype=np.int64)
    return ((i // 16 + 37 * (i % 16) + 11 * (i // 4096)) % 256).astype(np.uint8)


def _raw_into_guarded_buffer(src, table, in_dtype, out_dtype):
    """The raw entry point on a device copy of ``src`` (numpy uint8 [n]), its output in the middle of a sentinel-filled buffer ->
    (output bytes as numpy uint8 [n], launch name or None where nothing was launched); the sentinels are checked here."""
    from mct_quantizers_amd.hip import native
    lib = native.load()
    n = src.size
    code = {torch.uint8: native.CODE_U8, torch.int8: native.CODE_I8}
    dev = torch.from_numpy(src.copy()).cuda() if n else torch.zeros(16, dtype=torch.uint8, device="cuda")
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0 and dev.data_ptr() % 16 == 0 and table.data_ptr() % 4 == 0
    n0 = native.launch_count()
    rc = lib.mctq_codes_table(dev.data_ptr(), code[in_dtype], buf.data_ptr() + GUARD, code[out_dtype], n, table.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launched = native.launch_count() - n0
    assert launched == (1 if n else 0)
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + n:] == SENTINEL), n
    return got[GUARD:GUARD + n], (native.last_launch() if launched else None)


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", CHUNKS)
def test_codes_table_kernel_equals_the_cpu_route_at_every_path_size(chunks):
    from mct_quantizers_amd.hip import native, ops
    S = covered(chunks)
    table = permutation_table()
    dev_table = table.cuda()
    pairs = [(torch.uint8, torch.uint8), (torch.int8, torch.int8), (torch.uint8, torch.int8), (torch.int8, torch.uint8)]
    seen = set()
    native.set_tuning("table_chunks", chunks)
    try:
        for k, n in enumerate((0, 1, 15, 16, 17, 33, S - 1, S, S + 1, 2 * S + 21, 3 * S - 16)):
            src = every_byte_everywhere(n)
            in_dtype, out_dtype = pairs[k % 4]
            want = ops.codes_table(torch.from_numpy(src.copy()).view(in_dtype), table, out_dtype).view(torch.uint8).numpy()
            got, launch = _raw_into_guarded_buffer(src, dev_table, in_dtype, out_dtype)
            assert np.array_equal(got, want), (chunks, n)
            if n == 0:
                assert launch is None
                continue
            name = lambda dt: "i8" if dt == torch.int8 else "u8"                         # noqa: E731
            types = f"{name(in_dtype)} -> {name(out_dtype)}"
            assert launch.startswith(f"codes_table<{types} blocks={blocks_for(n, chunks)},"), (launch, n)
            assert f"U={chunks}," in launch and "in1B,out1B" in launch
            seen.add(types)
            if n >= 4096:                                    # every byte value at every position of a chunk
                assert all(len(np.unique(src[p:4096:16])) == 256 for p in range(16))
        assert seen == {"u8 -> u8", "i8 -> i8", "u8 -> i8", "i8 -> u8"}
        # the four type pairs give the same bytes: the table is indexed by the raw byte
        src = every_byte_everywhere(S + 21)
        outs = [_raw_into_guarded_buffer(src, dev_table, a, b)[0] for a, b in pairs]
        assert all(np.array_equal(o, outs[0]) for o in outs) and np.array_equal(outs[0], table.numpy()[src])
    finally:
        native.set_tuning("table_chunks", 4)


@pytest.mark.gpu
def test_the_workgroup_size_constant_is_the_launchers():
    """S as this file mirrors it against the block count in the launch note, one byte around each multiple."""
    from mct_quantizers_amd.hip import native
    dev_table = permutation_table().cuda()
    for chunks in CHUNKS:
        native.set_tuning("table_chunks", chunks)
        try:
            S = covered(chunks)
            for n, blocks in ((S, 1), (S + 15, 1), (S + 16, 2), (2 * S, 2), (2 * S + 16, 3)):
                _, launch = _raw_into_guarded_buffer(every_byte_everywhere(n), dev_table, torch.uint8, torch.uint8)
                assert f"blocks={blocks}," in launch and blocks == blocks_for(n, chunks), (chunks, n, launch)
        finally:
            native.set_tuning("table_chunks", 4)


@pytest.mark.gpu
def test_codes_table_refusals_come_before_any_launch():
    from mct_quantizers_amd.hip import native
    buf = torch.full((16384,), SENTINEL, dtype=torch.uint8, device="cuda")
    base = (buf.data_ptr() + 4096 + 255) // 256 * 256          # (the refusals' addresses reach 1024 bytes below and 4096 above)
    check_refusals(native.load(), native, base)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())                     # nothing was written


@pytest.mark.gpu
def test_codes_table_through_python_on_gpu_tensors():
    from mct_quantizers_amd.hip import native, ops
    from test_table_consumer import codes_of
    table = permutation_table()
    dev_table = table.cuda()
    for shape in ((0,), (1,), (15,), (17,), (2, 24, 7, 5), (3, 1031)):
        for in_dtype, out_dtype in ((torch.uint8, torch.int8), (torch.int8, torch.uint8)):
            codes = codes_of(shape, in_dtype)
            n0 = native.launch_count()
            y = ops.codes_table(codes.cuda(), dev_table, out_dtype)
            assert native.launch_count() - n0 == (1 if codes.numel() else 0)
            assert y.is_cuda and y.dtype == out_dtype and y.shape == codes.shape and y.stride() == codes.stride()
            assert torch.equal(y.cpu(), ops.codes_table(codes, table, out_dtype)), shape
    assert native.last_launch().startswith("codes_table<i8 -> u8 blocks=1,")
    # a view that is not dense, and one whose first byte is not 16-byte aligned: compacted first, the same bytes
    base = codes_of((4, 1031), torch.uint8).cuda()
    for view in (base[:, ::2], base[1:, 3:], base.reshape(-1)[5:4005]):
        assert torch.equal(ops.codes_table(view, dev_table, torch.uint8).cpu(), ops.codes_table(view.cpu(), table, torch.uint8))
    with pytest.raises(RuntimeError, match="the codes' device"):
        ops.codes_table(base, table, torch.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_the_module_gives_the_codes_of_the_float_chain_on_the_gpu(name):
    """The position-independence assumption, with strict equality: hb(f(ha(x))) in float32 on the device, coded by fq_codes,
    against QuantizedActivationTable(f, A, B)(x), for every accepted function, the four type pairs and three shapes."""
    from mct_quantizers_amd.hip import native
    for pair in HOLDER_PAIRS:
        q, fn, ha, hb = table_module(name, pair, "cuda")
        for shape in SHAPES:
            x = input_of(shape, "cuda")
            want, _, a_codes = float_chain(fn, ha, hb, x)
            y = q(x)                                         # (the first forward builds the table)
            assert y.dtype == want.dtype and y.shape == x.shape and torch.equal(y, want), (name, pair, shape)
            n0 = native.launch_count()
            again = q(a_codes)                               # A's codes in: the one launch
            assert native.launch_count() - n0 == 1 and native.last_launch().startswith("codes_table<"), (name, pair, shape)
            assert torch.equal(again, want)
        assert list(q._tables) == ["cuda:0"] and q.table("cuda:0").is_cuda


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["silu", "sigmoid", "gelu"])
@pytest.mark.parametrize("make", [MBConv, DecoderStage, TwoNodes])
def test_rewritten_blocks_give_the_bits_of_the_rewrite_without_the_switch_gpu(make, kind):
    from mct_quantizers_amd import consumers as C
    from mct_quantizers_amd.hip import native, ops
    build = lambda: make(kind)                               # noqa: E731
    args = model_args(make, "cuda")
    gm, n = rewritten(build, "cuda", **ALL)
    gm0, n0 = rewritten(build, "cuda", activation_tables=False, **ALL)
    cpu, _ = rewritten(build, "cpu", **ALL)
    tables = _table_nodes(gm)
    assert len(tables) == (2 if make is MBConv else 1) and sorted(tables) == sorted(_table_nodes(cpu)) and not _table_nodes(gm0)
    outs, outs_cpu, launches = {}, {}, {}

    def hooks_on(model, into, count=None):
        hs = []
        for name, m in _table_nodes(model).items():
            if count is not None:
                hs.append(m.register_forward_pre_hook(lambda m, a, name=name: count.__setitem__(name, native.launch_count())))
            hs.append(m.register_forward_hook(
                lambda m, a, out, name=name: into.__setitem__(name, (a[0], out, native.launch_count(), native.last_launch()))))
        return hs

    with torch.no_grad():
        gm(*args)                                            # (builds the tables)
        before = {}
        hs = hooks_on(gm, outs, before) + hooks_on(cpu, outs_cpu)
        y, y0 = gm(*args), gm0(*args)
        y_cpu = cpu(*[a.cpu() for a in args])
        for h in hs:
            h.remove()
    assert y.shape == y0.shape and len(torch.unique(y)) > 50 and torch.equal(y, y0)
    compared = 0
    for name, (operand, out, count, launch) in outs.items():
        # codes in, codes out, one launch
        assert operand.dtype in (torch.int8, torch.uint8) and out.dtype in (torch.int8, torch.uint8), name
        assert count - before[name] == 1 and launch.startswith("codes_table<"), (name, launch)
        # Against the CPU route of the same node, up to the CPU contract: the node IS its table on either device, and the two
        # tables are ATen's GPU and CPU evaluations of f on the same 256 values, which may differ in the last bits -- equal codes
        # wherever the two tables agree, at most one code apart (next to a rounding tie) elsewhere.
        operand_cpu, out_cpu, _, _ = outs_cpu[name]
        if not torch.equal(operand.cpu(), operand_cpu):
            continue                                         # (a table in front already differed by a code: nothing to compare)
        t_gpu, t_cpu = gm.get_submodule(name).table("cuda:0").cpu(), cpu.get_submodule(name).table("cpu")
        assert torch.equal(out_cpu, ops.codes_table(operand_cpu, t_cpu, out_cpu.dtype))
        same_entry = (t_gpu == t_cpu)[operand_cpu.view(torch.uint8).long()]
        diff = (out.cpu().to(torch.int32) - out_cpu.to(torch.int32)).abs()
        assert bool((diff[same_entry] == 0).all()) and int(diff.max()) <= 1, (name, int(diff.max()))
        as_codes = lambda t: t.view(out_cpu.dtype).to(torch.int32)                       # noqa: E731
        assert int((as_codes(t_gpu) - as_codes(t_cpu)).abs().max()) <= 1
        compared += 1
    assert y_cpu.shape == y.shape and compared >= 1


def _table_nodes(model):
    from mct_quantizers_amd import consumers as C
    return {name: m for name, m in model.named_modules() if isinstance(m, C.QuantizedActivationTable)}


@pytest.mark.gpu
def test_rewritten_mbconv_block_replays_from_a_hip_graph():
    import mct_quantizers_amd as mq
    gm, _ = rewritten(lambda: MBConv("silu"), "cuda", **ALL)
    x = model_args(MBConv, "cuda")[0]
    with torch.no_grad():
        captured = mq.capture_forward(gm, x, batch_weights=False)            # its warm-up forward builds the tables
        x2 = x * 0.5 + 0.25
        out = captured(x2).clone()
        eager = gm(x2)
        assert torch.equal(out, eager) and not torch.equal(out, gm(x)) and len(torch.unique(out)) > 50
