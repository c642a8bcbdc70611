"""tools/asm_same.py on two hand-written device assembly snippets: a kernel that differs only in
comments, label indices, directives and its own name is `same`; a changed instruction, or changed
kernel metadata, is `DIFF` and a non-zero exit status."""
import os
import subprocess
import sys

TOOL = os.path.join(os.path.dirname(__file__), "..", "tools", "asm_same.py")

ASM = """\
\t.text
\t.protected\t{name} ; -- Begin function {name}
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}: ; @{name}
; %bb.0:
\ts_load_dword s2, s[0:1], 0x0 {comment}
\ts_cbranch_scc1 .LBB{idx}_2

.LBB{idx}_1:
\t{insn}
.LBB{idx}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr 4
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{idx}:
\t.size\t{name}, .Lfunc_end{idx}-{name}
; codeLenInByte = 20
amdhsa.kernels:
  - .agpr_count:     0
    .group_segment_fixed_size: {lds}
    .name:           {name}
    .private_segment_fixed_size: 0
    .sgpr_count:     8
    .vgpr_count:     4
    .vgpr_spill_count: 0
"""


def _run(tmp_path, old, new, *maps):
    (tmp_path / "old.s").write_text(ASM.format(**old))
    (tmp_path / "new.s").write_text(ASM.format(**new))
    r = subprocess.run([sys.executable, TOOL, str(tmp_path / "old.s"), str(tmp_path / "new.s"), *maps],
                       capture_output=True, text=True)
    return r.returncode, r.stdout


OLD = dict(name="k_tILb1EE", idx=3, insn="v_add_f32_e32 v1, v2, v3", comment="; old comment", lds=1024)


def test_comments_labels_and_name_are_ignored(tmp_path):
    new = dict(OLD, name="k_t", idx=0, comment="")
    code, out = _run(tmp_path, OLD, new, "k_tILb1EE=k_t")
    assert code == 0, out
    assert "same  k_tILb1EE -> k_t" in out and "DIFF" not in out


def test_changed_instruction_is_a_diff(tmp_path):
    new = dict(OLD, name="k_t", idx=0, insn="v_sub_f32_e32 v1, v2, v3")
    code, out = _run(tmp_path, OLD, new, "k_tILb1EE=k_t")
    assert code != 0
    assert "DIFF  k_tILb1EE -> k_t" in out and "v_sub_f32_e32" in out


def test_changed_metadata_is_a_diff(tmp_path):
    code, out = _run(tmp_path, OLD, dict(OLD, lds=2048))
    assert code != 0
    assert "DIFF  k_tILb1EE" in out and "group_segment_fixed_size: 1024 -> 2048" in out


def test_a_side_may_be_several_listings(tmp_path):
    """k_a and k_b, one listing per kernel on either side, joined with `+`: both are found with their
    own metadata, and a change in the second listing is still a DIFF."""
    for name, text in (("old_a.s", dict(OLD, name="k_a")), ("old_b.s", dict(OLD, name="k_b", idx=4, lds=512)),
                       ("a.s", dict(OLD, name="k_a", idx=0))):
        (tmp_path / name).write_text(ASM.format(**text))
    for lds, want in ((512, 0), (256, 1)):
        (tmp_path / "b.s").write_text(ASM.format(**dict(OLD, name="k_b", idx=0, lds=lds)))
        r = subprocess.run([sys.executable, TOOL, f"{tmp_path / 'old_a.s'}+{tmp_path / 'old_b.s'}",
                            f"{tmp_path / 'a.s'}+{tmp_path / 'b.s'}"], capture_output=True, text=True)
        assert r.returncode == want, r.stdout
        assert "same  k_a" in r.stdout and ("same  k_b" if want == 0 else "DIFF  k_b") in r.stdout
        assert "2 -> 2 kernels" in r.stdout


def test_unmapped_kernel_is_gone_and_new(tmp_path):
    code, out = _run(tmp_path, OLD, dict(OLD, name="k_t"))
    assert code != 0
    assert "gone  k_tILb1EE" in out and "new   k_t" in out
