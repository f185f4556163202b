"""tools/kernel_diff.py OLD.s NEW.s : did a change move any kernel?  Reads two device assembly files (hipcc --save-temps:
msk_gpu-hip-amdgcn-amd-amdhsa-gfx950.s) and compares them kernel by kernel: the figures the compiler prints under "; Kernel info:"
(VGPRs, AGPRs, SGPRs, scratch, static LDS, occupancy, code length) and the kernel's text from its label to its end, descriptor
included, with comments taken out and the local labels (.LBB16_52, .Lfunc_end16: numbered by the function's position in the file)
renamed in order of appearance.  One line per kernel that differs or exists on one side only, exit status 1; "N kernels compared,
identical" and 0 otherwise.  It reads text and compares it: what the instructions are is none of its business."""
import re
import sys

FIGURES = {"NumVgprs": "vgpr", "NumAgprs": "agpr", "TotalNumSgprs": "sgpr", "ScratchSize": "scratch", "LDSByteSize": "lds",
           "Occupancy": "occ", "codeLenInByte": "bytes"}
_START = re.compile(r"^([A-Za-z_$][\w$.]*):")
_FIGURE = re.compile(r"^; (\w+)\s*[:=]\s*(\d+)")
_LABEL = re.compile(r"\.L[\w$.]+")


def kernels(text):
    """{symbol: (figures, normalised text)} of every function of `text` that carries a kernel descriptor"""
    out = {}
    name, lines, figs, is_kernel, in_text = None, [], {}, False, False

    def close():
        if name is not None and is_kernel:
            names = {}
            body = _LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), "\n".join(lines))
            out[name] = (figs, body)

    for line in text.splitlines():
        m = _START.match(line)
        if m:
            close()
            name, lines, figs, is_kernel, in_text = m.group(1), [], {}, False, True
        elif name is None:
            continue
        elif in_text:
            if line.startswith(".Lfunc_end"):
                in_text = False
                continue
            is_kernel = is_kernel or ".amdhsa_kernel" in line
            code = " ".join(line.split(";", 1)[0].split())
            if code:
                lines.append(code)
        else:
            f = _FIGURE.match(line)
            if f and f.group(1) in FIGURES:
                figs.setdefault(FIGURES[f.group(1)], int(f.group(2)))
    close()
    return out


def diff(old_text, new_text):
    """the lines to print: one per kernel that differs; the number of kernels compared"""
    old, new = kernels(old_text), kernels(new_text)
    report = []
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            report.append("%s: only in %s" % (k, "OLD" if k in old else "NEW"))
            continue
        (fo, to), (fn, tn) = old[k], new[k]
        what = ["%s %s -> %s" % (f, fo.get(f), fn.get(f)) for f in FIGURES.values() if fo.get(f) != fn.get(f)]
        if to != tn:
            what.append("text differs")
        if what:
            report.append("%s: %s" % (k, ", ".join(what)))
    return report, len(set(old) & set(new))


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    report, n = diff(open(sys.argv[1]).read(), open(sys.argv[2]).read())
    print("\n".join(report) if report else "%d kernels compared, identical" % n)
    sys.exit(1 if report else 0)
