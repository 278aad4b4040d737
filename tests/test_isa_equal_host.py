"""CPU: tools/isa_equal.py on three synthetic assembly texts -- equal files pass, comment-only changes pass, one changed operand is
reported against the kernel it is in."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "isa_equal.py")
NAME = "demo-hip-amdgcn-amd-amdhsa-gfx950.s"

BASE = """\t.text
\t.globl\t_Z10one_kernelPd
_Z10one_kernelPd:                       ; @_Z10one_kernelPd
; %bb.0:                                ; %entry
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v0, 0
.LBB0_1:                                ; %for.body.i
\tv_add_f64 v[2:3], v[2:3], v[4:5]
\ts_endpgm
.Lfunc_end0:
\t.size\t_Z10one_kernelPd, .Lfunc_end0-_Z10one_kernelPd
; NumVgprs: 6
\t.globl\t_Z10two_kernelPd
_Z10two_kernelPd:                       ; @_Z10two_kernelPd
; %bb.0:                                ; %entry
\tv_mul_f64 v[0:1], v[2:3], v[4:5]
\tv_fma_f64 v[0:1], v[0:1], v[2:3], v[4:5]
\ts_endpgm
.Lfunc_end1:
\t.size\t_Z10two_kernelPd, .Lfunc_end1-_Z10two_kernelPd
"""
# the block names one inlining level deeper, another figure in a comment line, blanks at a line's end: the same instruction stream
COMMENTS = BASE.replace("%for.body.i", "%for.body.i.i").replace("; NumVgprs: 6\n", "; NumVgprs: 8 \n").replace(
    "\ts_endpgm\n", "\ts_endpgm  \t\n")
# one operand of the second kernel
OPERAND = BASE.replace("v_fma_f64 v[0:1], v[0:1], v[2:3], v[4:5]", "v_fma_f64 v[0:1], v[0:1], v[2:3], v[6:7]")


def run(tmp_path, a, b):
    for side, text in (("a", a), ("b", b)):
        os.makedirs(tmp_path / side, exist_ok=True)
        if text is not None:
            (tmp_path / side / NAME).write_text(text)
    return subprocess.run([sys.executable, TOOL, str(tmp_path / "a"), str(tmp_path / "b")], capture_output=True, text=True)


def test_equal_files_pass(tmp_path):
    r = run(tmp_path, BASE, BASE)
    assert r.returncode == 0 and r.stdout.split() == ["SAME", NAME], r.stdout + r.stderr


def test_comment_only_changes_pass(tmp_path):
    assert COMMENTS != BASE
    r = run(tmp_path, BASE, COMMENTS)
    assert r.returncode == 0 and r.stdout.split() == ["SAME", NAME], r.stdout + r.stderr


def test_a_changed_operand_is_reported_against_its_kernel(tmp_path):
    r = run(tmp_path, BASE, OPERAND)
    assert r.returncode != 0, r.stdout
    lines = r.stdout.strip().split("\n")
    assert lines[0].split() == ["DIFF", NAME]
    assert len(lines) == 2 and "_Z10two_kernelPd: 3 -> 3 instructions" in lines[1] and "one_kernel" not in r.stdout, r.stdout


def test_a_file_missing_from_one_side_fails(tmp_path):
    r = run(tmp_path, BASE, None)
    assert r.returncode != 0 and "MISSING" in r.stdout and NAME in r.stdout, r.stdout
