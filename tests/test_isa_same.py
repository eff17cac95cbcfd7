"""tools/isa_same.py on two short synthetic listings: block-label numbers and the __hip_cuid_ symbol do not count as a
difference; one changed instruction does, and is reported with its function's symbol and both sides' figures."""
import importlib.util
import io
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("fqg_isa_same_module", os.path.join(REPO, "tools", "isa_same.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _function(name, n, body, vgprs=8):
    return f"""\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}: ; @{name}
; %bb.0:
{body}\ts_endpgm
.Lfunc_end{n}:
\t.size\t{name}, .Lfunc_end{n}-{name}
; Kernel info:
; NumVgprs: {vgprs}
; ScratchSize: 0
; Occupancy: 8
; LDSByteSize: 512 bytes/workgroup (compile time only)
"""


def _listing(first_fn, cuid, second_op="v_add_u32_e32 v1, v0, v0"):
    n = first_fn
    loop = f"""\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v0, 0
.LBB{n}_1: ; =>This Inner Loop Header: Depth=1
\t{second_op}
\tds_write_b32 v0, v1
\ts_cbranch_scc1 .LBB{n}_1
\tglobal_store_dword v0, v1, s[0:1]
"""
    other = f"""\tv_mov_b32_e32 v0, 1
\ts_cbranch_execz .LBB{n + 1}_2
\tglobal_store_dword v0, v0, s[0:1]
.LBB{n + 1}_2:
"""
    meta = "".join(f"""  - .group_segment_fixed_size: 512
    .name:           {name}
    .private_segment_fixed_size: 0
    .sgpr_count:     12
    .vgpr_count:     8
""" for name in ("_Z6k_loopPj", "_Z7k_otherPj"))
    return (_function("_Z6k_loopPj", n, loop) + _function("_Z7k_otherPj", n + 1, other) +
            f"\t.type\t__hip_cuid_{cuid},@object\n__hip_cuid_{cuid}:\n\t.byte\t0\n" +
            "amdhsa.kernels:\n" + meta + "...\n")


def test_label_numbers_and_cuid_are_no_difference():
    t = _tool()
    out = io.StringIO()
    assert t.compare(_listing(0, "1a2b3c"), _listing(7, "ffee00"), out) == []
    assert out.getvalue() == "2 of 2 device functions identical\n"


def test_one_changed_instruction_is_reported_with_its_symbol():
    t = _tool()
    out = io.StringIO()
    differ = t.compare(_listing(0, "1a2b3c"), _listing(0, "1a2b3c", "v_add3_u32 v1, v0, v0, s2"), out)
    assert differ == ["_Z6k_loopPj"]
    lines = out.getvalue().splitlines()
    assert lines[0] == "1 of 2 device functions identical"
    assert lines[1] == "== _Z6k_loopPj"
    for side in lines[2:4]:
        assert "valu 2, salu 3, vmem 1, lds 1, other 0" in side
        assert "vgpr 8, sgpr 12, scratch 0, lds 512, occupancy 8" in side
    assert len(lines) == 4


def test_a_function_on_one_side_only_is_reported():
    t = _tool()
    a = _listing(0, "1a2b3c")
    b = a.replace("_Z7k_otherPj", "_Z7k_otherPi")
    out = io.StringIO()
    assert sorted(t.compare(a, b, out)) == ["_Z7k_otherPi", "_Z7k_otherPj"]
    assert "not there" in out.getvalue()
