"""The compiled code of rows_kernel_finetail (csrc/mctq_kernels.hpp; tuning key "filldrain"), checked without a GPU: hipcc
cross-compiles the affine translation unit for gfx950 with the shipped flags, and on the ISA and the resource remarks of both
instances (non-temporal / cached stores): no scratch, no LDS, at most 64 VGPRs (8 waves per SIMD), the kernel arguments up to
the launch geometry preloaded into scalar registers, and on BOTH branches of the kernel -- the four-vector tile and the
one-vector piece of the fine tail -- the data loads issued ahead of the first wait on the row's scale (the scalar load of the
parameter fetch), the reciprocal behind them.  That order is what the route was measured with (profiles/EXPERIMENTS.md round 7):
a scale that is WAITED for in front of the data loads, or fetched by a vector load that returns in order behind them, delays
every block of the launch."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO

NAMES = ["_ZN4mctq20rows_kernel_finetailIffLi1EEEvPKT_PT0_PKfjjjjNS_8AffineOpE",       # <float, float, NT = 1>
         "_ZN4mctq20rows_kernel_finetailIffLi2EEEvPKT_PT0_PKfjjjjNS_8AffineOpE"]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    from mct_quantizers_amd.hip import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("finetail") / "affine.s"
    r = subprocess.run([hipcc, *B.FLAGS, "-I", os.path.join(REPO, "include"), "-I", B.CSRC, "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(asm), os.path.join(B.CSRC, "mctq_affine.hip")],
                       check=True, capture_output=True, text=True)
    return asm.read_text(), r.stderr


def _blocks(text, name):
    """the kernel's basic blocks in layout order (lists of instructions), the kernel-argument preload header left out"""
    body = text[text.index(name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    lines = [ln.split(";")[0].strip() for ln in body.splitlines()]
    lines = [ln for ln in lines if ln and (not ln.startswith(".") or re.match(r"\.LBB\d+_\d+:", ln)) and ln != name + ":"]
    blocks, cur = [], []
    for ln in lines:
        if re.match(r"\.LBB\d+_\d+:", ln):
            blocks.append(cur)
            cur = []
            continue
        cur.append(ln)
        if ln.startswith(("s_cbranch", "s_branch", "s_endpgm")):
            blocks.append(cur)
            cur = []
    blocks.append(cur)
    blocks = [b for b in blocks if b]
    # (the header: scalar loads of the arguments for a loader without preload support, one wait, a branch over the padding)
    assert blocks[0][-1].startswith("s_branch") and all(x.startswith(("s_load_dword", "s_waitcnt", "s_branch")) for x in blocks[0]), blocks[0]
    return blocks[1:]


@pytest.mark.parametrize("name", NAMES)
def test_resources(compiled, name):
    text, remarks = compiled
    assert name + ":" in text, f"{name} is not instantiated"
    vgpr = re.search(re.escape(name) + r"\.num_vgpr, (\d+)", text)
    agpr = re.search(re.escape(name) + r"\.num_agpr, (\d+)", text)
    scratch = re.search(re.escape(name) + r"\.private_seg_size, (\d+)", text)
    assert vgpr and int(vgpr.group(1)) <= 64 and agpr and int(agpr.group(1)) == 0, (vgpr and vgpr.group(1), agpr and agpr.group(1))
    assert scratch and int(scratch.group(1)) == 0, scratch and scratch.group(1)
    ins = [x for b in _blocks(text, name) for x in b]
    assert not [x for x in ins if x.startswith(("scratch_", "ds_", "buffer_"))]
    # the compiler's own remarks say the same
    rem = remarks[remarks.index("Function Name: " + name):]
    rem = rem[:rem.index("Function Name: ", 20)] if "Function Name: " in rem[20:] else rem
    assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", rem) and re.search(r"LDS Size \[bytes/block\]: 0\b", rem), rem[:1500]
    m = re.search(r"VGPRs: (\d+)", rem)
    assert m and int(m.group(1)) <= 64, rem[:1500]
    m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", rem)
    assert m and int(m.group(1)) == 8, rem[:1500]
    # xs, ys, scales and the four words of launch geometry arrive preloaded (10 dwords), as the build asks (hip/build.py)
    meta = text[text.index(".amdhsa_kernel " + name):]
    m = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", meta[:meta.index(".end_amdhsa_kernel")])
    assert m and int(m.group(1)) >= 10, m and m.group(1)


@pytest.mark.parametrize("name", NAMES)
def test_data_loads_are_issued_ahead_of_the_wait_for_the_scale(compiled, name):
    text, _ = compiled
    blocks = _blocks(text, name)
    is_data = lambda x: x.startswith("global_load_dwordx4")
    is_lgkm_wait = lambda x: x.startswith("s_waitcnt") and "lgkmcnt" in x
    # the row's scale: ONE scalar load of one dword through the preloaded table pointer (kernel arguments come from s[0:1])
    table = [(i, j) for i, b in enumerate(blocks) for j, x in enumerate(b) if re.match(r"s_load_dword s\d+, s\[(?!0:1\])", x)]
    assert len(table) == 1, table
    assert not [x for b in blocks for x in b if x.startswith("global_load_dword ")], "a table element fetched by a vector load"
    ti, tj = table[0]
    loaders = [i for i, b in enumerate(blocks) if any(is_data(x) for x in b)]
    assert len(loaders) == 2 and min(loaders) > ti, (loaders, ti)       # the fine piece and the four-vector tile, behind the request
    assert sorted(sum(is_data(x) for x in blocks[i]) for i in loaders) == [1, 4]
    # no wait on a scalar load between the request and the data loads: not behind the request in its own block, not in a block
    # between it and a loading block, not in front of the loads inside the loading block
    assert not [x for x in blocks[ti][tj:] if is_lgkm_wait(x)], blocks[ti][tj:]
    for i in loaders:
        b = blocks[i]
        last = max(j for j, x in enumerate(b) if is_data(x))
        assert not [x for x in b[:last] if is_lgkm_wait(x)], f"{name}: the scale is waited for in front of the data loads"
        assert all(x.rstrip().endswith(" nt") for x in b if is_data(x)), "the loads are not non-temporal"
        # ... the wait and the IEEE reciprocal (1.0f / scale) behind them, every store behind that
        after = b[last + 1:]
        assert after and is_lgkm_wait(after[0]), after[:3]
        rcp = [j for j, x in enumerate(after) if x.startswith("v_rcp_f32")]
        fix = [j for j, x in enumerate(after) if x.startswith("v_div_fixup_f32")]
        stores = [j for j, x in enumerate(after) if x.startswith("global_store_dwordx4")]
        assert len(rcp) == 1 and len(fix) == 1 and len(stores) == sum(is_data(x) for x in b) and fix[0] < stores[0], (rcp, fix, stores)
        before = [x for k, bb in enumerate(blocks[:i]) if k not in loaders for x in bb] + b[:last]
        assert not [x for x in before if x.startswith(("v_rcp_f32", "v_div_"))], "a reciprocal in front of the loads"
    for i in range(ti + 1, max(loaders)):
        if i not in loaders:
            assert not [x for x in blocks[i] if is_lgkm_wait(x)], (i, blocks[i])
    # per element the headline kernel's arithmetic: x * inv, round to nearest even, clamp, * s + 0
    for i in loaders:
        n = 4 * sum(is_data(x) for x in blocks[i])
        count = lambda pat: sum(bool(re.match(pat, x)) for x in blocks[i])
        assert count(r"v_rndne_f32") == n and count(r"v_med3_f32") == n and count(r"v_fma_f32 v\d+, v\d+, s\d+, 0$") == n, (i, n)
