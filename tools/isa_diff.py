#!/usr/bin/env python3
"""Compare kernels of two AMDGPU assembly files (hipcc --cuda-device-only -S), instruction for instruction.

    python3 tools/isa_diff.py OLD.s NEW.s 'attn_fwd_kernel<8,1,true,false,false>=attn_fwd_kernel<false,false>' attn_combine_kernel ...

Each pair is OLD=NEW (or one word for both): substrings of the demangled kernel names, spaces ignored; each must match exactly
one kernel of its file.  Per pair, the instruction streams (comments and directives dropped, the kernel's own symbol and its
labels renamed by order of definition) and the descriptor values (the .amdhsa_* directives, and VGPR / AGPR / SGPR counts, LDS
bytes, private segment size and kernarg size of the metadata) must be equal.  One line per pair; exit status 1 on any difference.
"""
import re
import shutil
import subprocess
import sys

META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".kernarg_segment_size")
LABEL_DEF = re.compile(r"^([A-Za-z_.$][\w.$]*):")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: d.replace(" ", "") for n, d in zip(names, out)}


def parse(path):
    """{symbol: (instructions, descriptor)} for every kernel of the file."""
    lines = open(path).read().split("\n")
    meta, cur = {}, None
    for ln in lines[lines.index("amdhsa.kernels:") + 1:] if "amdhsa.kernels:" in lines else []:
        if not ln.startswith("  "):
            break
        if ln.startswith("  - "):
            cur = {}
        m = re.match(r"^(?:  - |    )(\.\w+):\s+(\S+)$", ln)
        if m:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == ".name":
                meta[m.group(2)] = cur
    kernels = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)$", ln)
        if not m:
            continue
        sym = m.group(1)
        start = max(j for j in range(i) if lines[j].startswith(sym + ":"))
        code = [c.split(";")[0].strip() for c in lines[start + 1:i]]
        code = [c for c in code if c and (not c.startswith(".") or LABEL_DEF.match(c))]
        labels = {}
        for c in code:
            d = LABEL_DEF.match(c)
            if d:
                labels[d.group(1)] = "L%d" % len(labels)
        word = re.compile(r"(?<![\w.$])(" + "|".join(map(re.escape, [sym] + sorted(labels, key=len, reverse=True))) + r")(?![\w$])")
        code = [word.sub(lambda w: labels.get(w.group(1), "SELF"), c) for c in code]
        end = next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])
        desc = [" ".join(d.split()) for d in lines[i + 1:end]]
        desc += ["%s %s" % (k, meta[sym][k]) for k in META_KEYS]
        kernels[sym] = (code, desc)
    return kernels


def pick(kernels, names, want, path):
    hits = [s for s in kernels if want.replace(" ", "") in names[s]]
    if len(hits) != 1:
        sys.exit("%s: '%s' matches %d kernels of %s" % (sys.argv[0], want, len(hits), sorted(names[s] for s in kernels)))
    return hits[0]


def short(name):
    m = re.search(r"::(\w+(?:<[^>]*>)?)\(", name)
    return m.group(1) if m else name


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    old, new = parse(sys.argv[1]), parse(sys.argv[2])
    old_names, new_names = demangle(list(old)), demangle(list(new))
    bad = 0
    for pair in sys.argv[3:]:
        a, _, b = pair.partition("=")
        so, sn = pick(old, old_names, a, sys.argv[1]), pick(new, new_names, b or a, sys.argv[2])
        (co, do), (cn, dn) = old[so], new[sn]
        facts = dict(d.rsplit(" ", 1) for d in dn)
        what = []
        if co != cn:
            at = next((i for i, (x, y) in enumerate(zip(co, cn)) if x != y), min(len(co), len(cn)))
            what.append("instructions differ from #%d (%d vs %d): '%s' vs '%s'"
                        % (at, len(co), len(cn), co[at] if at < len(co) else "<end>", cn[at] if at < len(cn) else "<end>"))
        what += ["%s -> %s" % (x, y.rsplit(" ", 1)[1]) for x, y in zip(do, dn) if x != y]
        bad += bool(what)
        print("%-9s %s -> %s: %d instructions, vgpr %s agpr %s sgpr %s lds %s scratch %s kernarg %s%s"
              % ("DIFFERENT" if what else "identical", short(old_names[so]), short(new_names[sn]), len(cn),
                 *(facts[k] for k in META_KEYS), "".join("\n    " + w for w in what)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
