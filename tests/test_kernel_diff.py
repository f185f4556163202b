"""tools/kernel_diff.py: the comparison a change that must not move a kernel is held to (EXPERIMENTS.md, "Name each shading family
once") — two device assembly texts, kernel by kernel: the compiler's figures and the text, local labels renamed.  CPU only."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "kernel_diff.py")

# a kernel as the compiler writes one: label, text with local labels that carry the function's index, descriptor, end label, figures
KERNEL = """\
\t.text
\t.globl\t{name}
\t.type\t{name},@function
{name}:                                 ; @{name}
; %bb.0:
\ts_load_dword s3, s[0:1], 0x2e8
\ts_cbranch_scc1 .LBB{idx}_2
.LBB{idx}_1:                              ; =>This Inner Loop Header: Depth=1
\tv_add_u32_e32 v1, s3, v0
\ts_cbranch_vccnz .LBB{idx}_1
.LBB{idx}_2:                              ; %.loopexit
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr {vgpr}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{idx}:
\t.size\t{name}, .Lfunc_end{idx}-{name}
; Kernel info:
; codeLenInByte = 24
; TotalNumSgprs: 10
; NumVgprs: {vgpr}
; NumAgprs: 0
; ScratchSize: 0
; LDSByteSize: 0 bytes/workgroup (compile time only)
; Occupancy: 8
"""


def _asm(*kernels):
    return "".join(KERNEL.format(name=n, idx=i, vgpr=v) for n, i, v in kernels)


def _run(tmp_path, old, new):
    a, b = tmp_path / "old.s", tmp_path / "new.s"
    a.write_text(old)
    b.write_text(new)
    return subprocess.run([sys.executable, TOOL, str(a), str(b)], capture_output=True, text=True)


def test_kernel_diff_equal_apart_from_labels_and_differing_in_a_register_count(tmp_path):
    # the same two kernels emitted in the other order: every local label carries another index, nothing else differs
    old = _asm(("k_one", 0, 2), ("k_two", 1, 2))
    r = _run(tmp_path, old, _asm(("k_two", 0, 2), ("k_one", 1, 2)))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "2 kernels compared, identical"
    # one register more in k_two: its figure and its descriptor differ; k_one is not reported
    r = _run(tmp_path, old, _asm(("k_one", 0, 2), ("k_two", 1, 3)))
    assert r.returncode == 1
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("k_two: ") and "vgpr 2 -> 3" in lines[0] and "text differs" in lines[0]
    # a kernel that exists on one side only is a difference too
    r = _run(tmp_path, old, _asm(("k_one", 0, 2)))
    assert r.returncode == 1 and r.stdout.strip() == "k_two: only in OLD"

