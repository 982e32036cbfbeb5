"""What the shipped 256 x 192 pipelined bf16 GEMM kernels do between their last MFMA and their first output store, read off the
gfx950 code object inside the built library (no GPU needed): the matrix pipe is idle there, so a global-memory round trip in
that stretch is paid in full, 19 times per C3 step.  The epilogue's operands are parked in LDS at kernel entry
instead (bias slice, 1-bit ReLU mask tile), the next launch's weights are touched but not waited for, and the barriers are raw
s_barrier, which drains nothing.  This test keeps it that way:

  * no global / buffer load into registers in that stretch other than the next-weights touch (one global_load_dword) and, for
    the fused-loss kernel, its target-row and mask-table gathers;
  * no `s_waitcnt vmcnt` there other than the one drain of the LDS-DMA queue behind the K loop (fused loss: its gathers' own waits,
    none of them before the first gather is issued);
  * the 1-bit-mask data gradient (an instantiation of its own) holds no vmcnt wait and no load up to its LAST output store - only
    the instantiation that masks by the saved activation (CODAE_NO_RELU_BITS=1) loads, 13 rows in flight together, and waits.

The code is taken in address order, as tools/check_isa.py takes it.
"""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_isa():
    spec = importlib.util.spec_from_file_location("codae_check_isa", os.path.join(ROOT, "tools", "check_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def kernels():
    """{(nlb, a_mode, b_mode, c_f32, epi, pol) or ('grouped', n): instructions behind the last MFMA} of the 256 x 192 instantiations
    that ship (DBG = 0)"""
    C = _check_isa()
    if not os.path.exists(C.DEFAULT_LIB):
        pytest.skip("libcodae_hip.so is not built")
    if not os.path.exists(os.path.join(C.LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump not found")
    funcs = C.functions(C.disassemble(C.DEFAULT_LIB))
    out = {}
    n_grouped = 0
    for name, insns in funcs.items():
        mfma = [i for i, (_, o, _) in enumerate(insns) if o.startswith("v_mfma")]
        if not mfma:
            continue
        tail = [(o, a) for _, o, a in insns[mfma[-1] + 1:]]
        if "gemm_bf16_pipe_grouped_kernel" in name:
            out[("grouped", n_grouped)] = tail
            n_grouped += 1
            continue
        m = re.search(r"gemm_bf16_pipe_kernelI((?:L[ib]\d+E)+)E", name)
        if not m:
            continue
        t = [int(x) for x in re.findall(r"L[ib](\d+)E", m.group(1))]
        bm, bn, _, _, nlb, am, bmode, cf, dbg, epi, pol = t
        if (bm, bn) == (256, 192) and dbg == 0:
            out[(nlb, am, bmode, cf, epi, pol)] = tail
    return out


def is_load(op):
    return op.startswith(("global_load", "buffer_load", "flat_load")) and not op.startswith("global_load_lds")


def is_out_store(op):
    return op in ("global_store_dwordx4", "buffer_store_dwordx4")


def is_vm_wait(op, args):
    return op == "s_waitcnt" and "vmcnt" in args


def before_first_store(tail):
    first = next(i for i, (o, _) in enumerate(tail) if is_out_store(o))
    return tail[:first]


def pick(kernels, want):
    got = {k: v for k, v in kernels.items() if want(k)}
    assert got, "no such instantiation in the library"
    return got


def assert_only_the_drain(key, stretch, touch_allowed):
    loads = [o for o, _ in stretch if is_load(o)]
    assert loads in ([], ["global_load_dword"][:touch_allowed]), (key, loads)
    waits = [a for o, a in stretch if is_vm_wait(o, a)]
    assert waits == ["vmcnt(0)"], (key, waits)


def test_forward_kernels_issue_their_first_store_behind_one_drain(kernels):
    ks = pick(kernels, lambda k: k[0] != "grouped" and k[3] == 0 and k[4] == 1)
    assert {k[5] for k in ks} == {0, 1}, "both store policies"
    for key, tail in ks.items():
        assert_only_the_drain(key, before_first_store(tail), 1)


def test_fp32_and_grouped_weight_gradient_kernels_load_nothing_in_the_epilogue(kernels):
    ks = pick(kernels, lambda k: k[0] == "grouped" or k[3] == 1)
    assert sum(1 for k in ks if k[0] == "grouped") == 2, "grouped kernel: both store policies"
    assert {k[5] for k in ks if k[0] != "grouped"} == {0, 1}
    for key, tail in ks.items():
        assert_only_the_drain(key, before_first_store(tail), 1)
        # (and neither row half's stores are waited for: the staging of the second half follows a raw barrier)
        last = max(i for i, (o, _) in enumerate(tail) if is_out_store(o))
        assert [a for o, a in tail[:last] if is_vm_wait(o, a)] == ["vmcnt(0)"], key


def test_one_bit_mask_data_gradient_kernels_wait_for_nothing_up_to_their_last_store(kernels):
    """EPI 4: the data gradient behind a forward launch that left 1-bit masks - the C3 step's nine"""
    ks = pick(kernels, lambda k: k[0] != "grouped" and k[3] == 0 and k[4] == 4)
    assert {k[5] for k in ks} == {0, 1}
    rows_per_thread = 13                       # 256 rows / (512 threads / 24 16-B chunks per row), rounded up
    for key, tail in ks.items():
        stores = [i for i, (o, _) in enumerate(tail) if is_out_store(o)]
        assert len(stores) == rows_per_thread, (key, len(stores))
        upto = tail[:stores[-1] + 1]
        assert_only_the_drain(key, upto, 1)
        assert any(o in ("ds_read_u8", "ds_read_i8") for o, _ in upto), (key, "the mask bytes come from LDS")


def test_activation_mask_data_gradient_kernels_keep_their_loads_behind_the_staging(kernels):
    """EPI 2 (CODAE_NO_RELU_BITS=1, k-strided operand forms): up to its first store no copy of the write-out waits for more than the
    drain; the copy that masks by the saved activation has its 13 rows in flight together"""
    ks = pick(kernels, lambda k: k[0] != "grouped" and k[3] == 0 and k[4] == 2)
    assert {k[5] for k in ks} == {0, 1}
    for key, tail in ks.items():
        assert_only_the_drain(key, before_first_store(tail), 1)
        assert sum(1 for o, _ in tail if o == "global_load_dwordx4") == 13, key


def test_fused_loss_kernels_wait_for_nothing_but_their_gathers(kernels):
    ks = pick(kernels, lambda k: k[0] != "grouped" and k[4] == 3)
    assert {k[5] for k in ks} == {0, 1}
    for key, tail in ks.items():
        stretch = before_first_store(tail)
        loads = [(i, o) for i, (o, _) in enumerate(stretch) if is_load(o)]
        assert {o for _, o in loads} <= {"global_load_dword", "global_load_dwordx4"}, key      # touch + mask bytes; target rows
        first_gather = next(i for i, o in loads if o == "global_load_dwordx4")
        # no bias loads: every 16-B load is a target-row gather, 24 per row half of a wave (2 x 6 column groups x 2 row tiles) ...
        assert sum(1 for _, o in loads if o == "global_load_dwordx4") == 48, key
        # ... and nothing is waited for between the drain and the first gather: the touch is not, the bias comes from LDS
        assert [a for o, a in stretch[:first_gather] if is_vm_wait(o, a)] == ["vmcnt(0)"], key
