"""tools/isa_compare.py: the splitter and the normaliser, on made-up assembly text
(no GPU, no compiler)."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "isa_compare", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "isa_compare.py"))
ic = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ic)


def func(name, index, body):
    """One function as the compiler lays it out; `index` is its place in the file."""
    return f"""\t.protected\t{name} ; -- Begin function {name}
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}: ; @{name}
; %bb.0:
{body.replace("#", str(index))}
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr 9
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{index}:
\t.size\t{name}, .Lfunc_end{index}-{name}
                                        ; -- End function
\t.set {name}.num_vgpr, 9
; Kernel info:
; codeLenInByte = 44
"""


HEAD = '\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"\n\t.text\n'
LOOP = """\ts_mov_b32 s0, 0 ; a comment
.LBB#_1: ; =>This Inner Loop Header: Depth=1
\ts_add_u32 s0, s0, 1
\ts_cmp_lt_u32 s0, 64
\ts_cbranch_scc1 .LBB#_1"""
TAIL = "\t.type\t__hip_cuid_{0},@object\n\t.globl\t__hip_cuid_{0}\n__hip_cuid_{0}:\n\t.byte\t0\n\t.size\t__hip_cuid_{0}, 1\n"


def test_two_functions():
    f = ic.split_functions(HEAD + func("_Z1av", 0, LOOP) + func("_Z1bv", 1, "\tv_mov_b32 v0, 0") + TAIL.format("ab12"))
    assert list(f) == ["_Z1av", "_Z1bv"]
    assert f["_Z1av"][0] == ".type _Z1av,@function" and f["_Z1av"][-1] == ".set _Z1av.num_vgpr, 9"
    assert "s_mov_b32 s0, 0" in f["_Z1av"] and ".amdhsa_next_free_vgpr 9" in f["_Z1av"]
    assert "v_mov_b32 v0, 0" in f["_Z1bv"] and "v_mov_b32 v0, 0" not in f["_Z1av"]
    assert not any(";" in line for lines in f.values() for line in lines)


def test_renumbered_labels():
    # the same function second in one file and first in the other, the unit ids different
    old = ic.split_functions(HEAD + func("_Z1bv", 0, "\tv_mov_b32 v0, 0") + func("_Z1av", 1, LOOP) + TAIL.format("ab12"))
    new = ic.split_functions(HEAD + func("_Z1av", 0, LOOP) + TAIL.format("cd34"))
    assert ic.compare(old, new) == [("_Z1bv", "only in old"), ("_Z1av", f"IDENTICAL ({len(new['_Z1av'])} lines)")]
    assert ic.normalise("\ts_cbranch_scc1 .LBB17_3 ; x") == "s_cbranch_scc1 .LBB_3"
    assert ic.normalise("\ts_cbranch_scc1 .LBB17_3") != ic.normalise("\ts_cbranch_scc1 .LBB17_4")
    assert ic.normalise("__hip_cuid_0123abcd:") == ic.normalise("__hip_cuid_fedc9876:")


def test_changed_instruction():
    old = ic.split_functions(HEAD + func("_Z1av", 0, LOOP) + func("_Z1bv", 1, "\tv_mov_b32 v0, 0"))
    new = ic.split_functions(HEAD + func("_Z1av", 0, LOOP.replace("s0, 64", "s0, 65")) + func("_Z1bv", 1, "\tv_mov_b32 v0, 0"))
    v = dict(ic.compare(old, new))
    assert v["_Z1av"] == "DIFFERENT" and v["_Z1bv"].startswith("IDENTICAL")
    # a changed register is a change too
    new = ic.split_functions(HEAD + func("_Z1av", 0, LOOP.replace("s0", "s1")))
    assert dict(ic.compare(old, new))["_Z1av"] == "DIFFERENT"
    assert ic.allowed("a()", ["a"]) and ic.allowed("a()", ["a()"]) and not ic.allowed("ab()", ["a"])


def test_function_missing_on_one_side():
    both = func("_Z1av", 0, LOOP)
    old = ic.split_functions(HEAD + both + func("_Z1bv", 1, "\tv_mov_b32 v0, 0"))
    new = ic.split_functions(HEAD + both + func("_Z1cv", 1, "\tv_mov_b32 v0, 0"))
    assert [v for _, v in ic.compare(old, new)] == [f"IDENTICAL ({len(old['_Z1av'])} lines)", "only in old", "only in new"]
    assert [s for s, _ in ic.compare(old, new)] == ["_Z1av", "_Z1bv", "_Z1cv"]
