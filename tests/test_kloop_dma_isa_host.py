"""How the pipelined bf16 GEMM kernels address their LDS-DMA pieces inside the K loop, read off the gfx950 code object inside the
built library (no GPU needed).

The design (gemm_bf16_halftile.h, half_src) hands every piece to the DMA instruction as {wave-uniform SGPR base, loop-invariant
32-bit lane offset}: `global_load_lds_dwordx4 v, s[..]`.  The compiler emits that form only while it can see, in the block of the
load, that the lane offset is a zero-extended 32-bit value; once the zero-extension is hoisted out of the loop it selects
`v_lshl_add_u64 v[..], s[..], 0, v[..]` + `global_load_lds_dwordx4 v[..], off` instead - a 64-bit VALU add per piece on the loader
wave, on the instructions measured to be the exposed cost of the K loop, and twice the address registers.  This test keeps the
scalar-base form in every K-loop block of every shipped instantiation.

A K-loop block is a basic block (code between branches and branch targets, in address order as tools/check_isa.py takes it) with at
least 48 MFMAs and at least one LDS-DMA: for the 256-row tiles the two-K-tile loop bodies (96 MFMAs) and the odd-count tail K-tile
(48) of the loader waves, for the 128 x 192 tile its loop bodies (48).
"""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DMA = "global_load_lds_dwordx4"
ADD64 = ("v_lshl_add_u64", "v_add_co_u32", "v_addc_co_u32", "v_add_co_ci_u32")


def _check_isa():
    spec = importlib.util.spec_from_file_location("codae_check_isa", os.path.join(ROOT, "tools", "check_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def basic_blocks(C, insns):
    """[[(address, mnemonic, operands)]]: split behind every branch and in front of every branch target"""
    base = insns[0][0]
    targets = set()
    for _, op, args in insns:
        if op.startswith("s_cbranch") or op == "s_branch":
            m = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>", args)
            if m:
                targets.add(base + int(m.group(1), 16))
    blocks, cur = [], []
    for ins in insns:
        if ins[0] in targets and cur:
            blocks.append(cur)
            cur = []
        cur.append(ins)
        if ins[1].startswith("s_cbranch") or ins[1] in ("s_branch", "s_endpgm"):
            blocks.append(cur)
            cur = []
    if cur:
        blocks.append(cur)
    return blocks


def kloop_blocks(C, insns):
    out = []
    for b in basic_blocks(C, insns):
        if sum(1 for _, o, _ in b if o.startswith("v_mfma")) >= 48 and any(o == DMA for _, o, _ in b):
            out.append(b)
    return out


@pytest.fixture(scope="module")
def pipelined():
    """{pretty kernel name: [K-loop blocks]} of every pipelined bf16 GEMM kernel in the library"""
    C = _check_isa()
    if not os.path.exists(C.DEFAULT_LIB):
        pytest.skip("libcodae_hip.so is not built")
    if not os.path.exists(os.path.join(C.LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump not found")
    funcs = C.functions(C.disassemble(C.DEFAULT_LIB))
    names = [n for n in funcs if "gemm_bf16_pipe_kernel" in n or "gemm_bf16_pipe_grouped_kernel" in n]
    out = {}
    for n in names:
        m = re.search(r"gemm_bf16_pipe_kernelI((?:L[ib]\d+E)+)E", n)
        pretty = "pipe<%s>" % ",".join(re.findall(r"L[ib](\d+)E", m.group(1))) if m else "grouped<%s>" % re.search(r"ILi(\d+)E", n).group(1)
        out[pretty] = kloop_blocks(C, funcs[n])
    return out


def test_every_instantiation_is_seen(pipelined):
    """both loader layouts of the 256 x 192 tile, the 128 x 192 tile and the grouped kernel, each with K-loop blocks of loader waves"""
    tiles = {tuple(k[5:-1].split(",")[i] for i in (0, 1, 4)) for k in pipelined if k.startswith("pipe<")}
    assert {("256", "192", "4"), ("256", "192", "6"), ("128", "192", "4")} <= tiles, tiles
    assert sum(1 for k in pipelined if k.startswith("grouped<")) == 2
    for k, blocks in pipelined.items():
        assert blocks, (k, "no K-loop block with LDS-DMA found")


def test_kloop_dma_takes_a_scalar_base_and_a_32_bit_lane_offset(pipelined):
    for k, blocks in pipelined.items():
        for b in blocks:
            bad = [(hex(a), ar) for a, o, ar in b if o == DMA and not re.match(r"^v\d+, s\[\d+:\d+\]", ar)]
            assert not bad, (k, len(bad), bad[:3])


def test_no_64_bit_add_feeds_a_kloop_dma(pipelined):
    """no v_lshl_add_u64 / v_add_co + v_addc pair in a K-loop block writes a register one of the block's LDS-DMA pieces reads"""
    C = _check_isa()
    for k, blocks in pipelined.items():
        for b in blocks:
            addr = set()
            for _, o, ar in b:
                if o == DMA:
                    addr |= C.regs_of(ar.split(",")[0])
            assert addr, k
            for a, o, ar in b:
                if o.startswith(ADD64):
                    assert not (C.regs_of(ar.split(",")[0]) & addr), (k, hex(a), o, ar)



def test_chain_kernel_weight_ring_takes_the_scalar_base_form_too():
    """chain_bf16.hip requests its weight units as {wave-uniform matrix position, 32-bit lane offset} as well: every LDS-DMA inside
    the kernel's multiply loops (innermost loops with MFMAs, as tools/check_isa.py finds them) has the scalar-base form"""
    C = _check_isa()
    if not os.path.exists(C.DEFAULT_LIB):
        pytest.skip("libcodae_hip.so is not built")
    if not os.path.exists(os.path.join(C.LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump not found")
    funcs = C.functions(C.disassemble(C.DEFAULT_LIB))
    chains = [ins for n, ins in funcs.items() if "chain_step_kernel" in n]
    assert chains
    for ins in chains:
        loads = [(hex(a), ar) for lo, hi in C.loops_with_mfma(ins) for a, o, ar in ins[lo:hi + 1] if o == DMA]
        assert len(loads) >= 2, "no weight-ring DMA found in the multiply loops"
        bad = [x for x in loads if not re.match(r"^v\d+, s\[\d+:\d+\]", x[1])]
        assert not bad, (len(bad), bad[:3])
