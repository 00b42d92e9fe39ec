"""tools/isa_digest.py's normaliser, on synthetic listings (no hipcc): the table it prints is how a refactor of csrc/ shows
that the device code did not change, so label numbers, comments and alignment directives — what moves when a kernel changes
files — must not reach a digest, and an operand must."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("isa_digest", os.path.join(ROOT, "tools", "isa_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _tool()

LISTING = """\t.text
\t.p2align\t8
\t.type\t_Z1kPf,@function
_Z1kPf:                                 ; @_Z1kPf
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v1, 0                     ; a comment
\ts_waitcnt lgkmcnt(0)
.LBB{f}_1:                                ; =>This Inner Loop Header: Depth=1
\t;;#ASMSTART
\tv_add_f32 v1, v1, {operand}
.Lloop_{a}:
\ts_cbranch_scc1 .Lloop_{a}
\t;;#ASMEND
\t.p2align\t6
\t.loc\t1 20 5
\ts_cbranch_vccnz .LBB{f}_1
; %bb.2:
\tglobal_store_dword v0, v1, s[0:1]
\ts_endpgm
.Lfunc_end{f}:
\t.size\t_Z1kPf, .Lfunc_end{f}-_Z1kPf
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel _Z1kPf
\t\t.amdhsa_next_free_vgpr {vgprs}
\t\t.amdhsa_next_free_sgpr 8
\t.end_amdhsa_kernel
"""


def digest(f=0, a=17, operand="v2", vgprs=3, strip=()):
    lines = [ln for ln in LISTING.format(f=f, a=a, operand=operand, vgprs=vgprs).split("\n") if not ln.strip().startswith(strip or "\0")]
    out = T.kernels(lines)
    assert list(out) == ["_Z1kPf"]
    return out["_Z1kPf"]


def test_label_numbers_comments_and_alignment_do_not_reach_the_digest():
    base = digest()
    assert base[0] == 8  # instructions: labels, directives, comments and asm markers are not counted
    assert digest(f=41, a=3) == base
    assert digest(strip=(".p2align", ".loc", "; %bb")) == base
    text, count = T.normalise(["\tv_mov_b32_e32 v1, 0   ; x", "", "\t.cfi_startproc", ".LBB7_2:", "\ts_branch .LBB7_2"])
    assert (text, count) == ("v_mov_b32_e32 v1, 0\n.L0:\ns_branch .L0", 2)


def test_a_changed_operand_or_register_block_changes_its_digest():
    count, stream, meta = digest()
    assert digest(operand="v3") == (count, digest(operand="v3")[1], meta) and digest(operand="v3")[1] != stream
    assert digest(vgprs=4)[1] == stream and digest(vgprs=4)[2] != meta
    # two labels that trade places are a different control flow, whatever their numbers
    swapped = T.normalise([".LA1:", ".LB2:", "\ts_branch .LB2"])[0]
    assert swapped != T.normalise([".LA1:", ".LB2:", "\ts_branch .LA1"])[0]


def test_compare_lists_missing_new_and_different_kernels():
    saved = ["# 3 kernels; hipcc x", "a()\t3\t11\t22", "b()\t3\t11\t22", "c()\t3\t11\t22"]
    assert T.compare(saved[1:], saved) == []
    diff = T.compare(["a()\t3\t11\t22", "b()\t4\t12\t22", "d()\t3\t11\t22"], saved)
    assert [d.split("\n")[0] for d in diff] == ["missing: c()", "new: d()", "different: b()"]
