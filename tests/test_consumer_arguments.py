"""The integer consumer's entry points refuse bad calls before they touch HIP (csrc/mctq_qlinear.hip: ql_check_call and
ql_output_form, shared by all six), so their argument checks run without a GPU: every call here is one the library
refuses, or an empty product -- nothing is ever launched and no pointer is ever dereferenced.  At most one fault per call:
which message a call with several faults gets is not part of the contract."""
import pytest

from mct_quantizers_amd.hip import build, native

E, I8, U8 = native.MCTQ_E_ARG, native.CODE_I8, native.CODE_U8
P = 4096                                        # an aligned address that is never dereferenced
LUT = bytes(range(16))                          # lut16 is a HOST pointer the library reads: a real buffer

# entry point -> the optional argument groups it has (hip/native.py: _ql_signature)
ENTRIES = {
    "mctq_qlinear_i8": dict(),
    "mctq_qlinear_i8_codes": dict(form=True),
    "mctq_qlinear_w4a8": dict(form=True, packed=True),
    "mctq_qlinear_lut4a8": dict(form=True, packed=True, lut=True),
    "mctq_qlinear_i8_zp": dict(form=True, zp=True),
    "mctq_qlinear_w4a8_zp": dict(form=True, packed=True, zp=True),
}
ALIGNMENT = {False: b"code matrices must be 16-byte aligned",
             True: b"a_codes must be 16-byte and the packed weights (w_codes4 / w_idx4) 8-byte aligned"}


@pytest.fixture(scope="module")
def lib():
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    lib = native.load()
    count = lib.mctq_launch_count()
    yield lib
    assert lib.mctq_launch_count() == count     # refused and empty calls launch nothing


def make_call(lib, name):
    """call(**overrides) -> rc of one consumer call whose arguments are all valid unless overridden."""
    groups = ENTRIES[name]
    # with an output form the default is a valid one (uint8 codes); mctq_qlinear_i8 has none
    valid = dict(a=P, adt=U8, za=3, sa=0.5, w=P, lut16=LUT, w_scales=P, w_rowsum=P, bias=None, y=P,
                 ydt=U8, y_scale=0.25, y_zp=0, qmin=0, qmax=255, zw=P, a_rowsum=P, M=4, N=8, K=64)

    def call(**overrides):
        v = dict(valid, **overrides)
        args = [v["a"], v["adt"], v["za"], v["sa"], v["w"]]
        if groups.get("lut"):
            args.append(v["lut16"])
        args += [v["w_scales"], v["w_rowsum"], v["bias"], v["y"]]
        if groups.get("form"):
            args += [v["ydt"], v["y_scale"], v["y_zp"], v["qmin"], v["qmax"]]
        if groups.get("zp"):
            args += [v["zw"], v["a_rowsum"]]
        return getattr(lib, name)(*args, v["M"], v["N"], v["K"], None)

    return call


@pytest.mark.parametrize("name", list(ENTRIES))
def test_consumer_entry_point_refuses_bad_arguments(lib, name):
    groups = ENTRIES[name]
    packed = bool(groups.get("packed"))
    call = make_call(lib, name)

    def refused(message, **fault):
        assert call(**fault) == E, (name, fault)
        assert lib.mctq_last_error() == message, (name, fault, lib.mctq_last_error())

    for extent in "MNK":
        refused(b"negative extent", **{extent: -1})
    refused(b"bad a_code_dtype", adt=77)
    refused(b"K must be a multiple of 16", K=24)
    refused(b"K > 32768 could overflow the int32 accumulator", K=65536)
    refused(ALIGNMENT[packed], a=P + 1)
    refused(ALIGNMENT[packed], w=P + 4)          # packed weights need 8 bytes, int8 weights 16: four off fits neither
    if packed:
        assert call(w=P + 8, M=0) == 0           # (eight off is aligned for them; an empty call, so nothing runs)
    else:
        refused(ALIGNMENT[packed], w=P + 8)
    for pointer in ("a", "w", "w_scales", "w_rowsum", "y"):
        refused(b"NULL pointer", **{pointer: None})
    refused(b"M or N too large", M=2 ** 31)
    refused(b"M or N too large", N=2 ** 31)
    if groups.get("zp"):
        refused(b"w_zero_points and a_rowsum are both required", a_rowsum=None)
        refused(b"w_zero_points and a_rowsum are both required", zw=None)
    if groups.get("lut"):
        refused(b"lut16 is NULL (a HOST pointer to 16 int8 codebook values)", lut16=None)
    if groups.get("form"):
        refused(b"bad y_code_dtype", ydt=9)
        refused(b"quant_min > quant_max", qmin=200, qmax=100)
        refused(b"clamp domain does not fit the code type", qmax=256)                   # uint8 codes: 0 .. 255
        refused(b"clamp domain does not fit the code type", ydt=I8, qmin=-129, qmax=127)
        refused(b"clamp domain does not fit the code type", ydt=I8, qmin=-128, qmax=128)
    if name == "mctq_qlinear_i8_codes":
        refused(b"bad y_code_dtype", ydt=-1)     # the other entry points read a negative y_code_dtype as float32


@pytest.mark.parametrize("name", list(ENTRIES))
def test_empty_consumer_call_returns_zero_before_any_pointer_check(lib, name):
    call = make_call(lib, name)
    nothing = dict(a=None, w=None, w_scales=None, w_rowsum=None, bias=None, y=None, zw=None, a_rowsum=None)
    assert call(M=0, **nothing) == 0
    assert call(N=0, **nothing) == 0
    if ENTRIES[name].get("form") and name != "mctq_qlinear_i8_codes":
        assert call(M=0, ydt=-1, **nothing) == 0                                        # float32 output form


def test_empty_codes_rowsum_returns_zero(lib):
    assert lib.mctq_codes_rowsum(None, U8, 3, None, 0, 64, None) == 0
    assert lib.mctq_codes_rowsum(P, U8, 3, P, -1, 64, None) == E and lib.mctq_last_error() == b"negative extent"
