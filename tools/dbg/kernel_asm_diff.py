"""Per-kernel identity of the gfx950 device code of attention sources between two trees: the check that an edit changed no
machine code when it changes the order in which kernels are emitted (text_md5.sh then differs) or the parameter types in
their mangled names.

    python tools/dbg/kernel_asm_diff.py OLD_TREE NEW_TREE [source.hip ...]   (default: the four attention sources)

Each source is compiled with the product flags (vorta_amd/build.py FLAGS, -S --cuda-device-only) in both trees; per kernel
the instruction stream (comments dropped, .LBB<fn>_<n> labels and the kernel's own symbol normalised) and the descriptor's
next_free_vgpr / next_free_sgpr / accum_offset / group and private segment sizes must be equal.  Kernels are matched by
name and template arguments without the parameter block's type; the split-key merges of the families (attn_combine_kernel
<T>, attn8_ / attn_mx_ / attn_i8_combine_kernel<T> before they were one template) by output type and parameter block.
Exit status 1 on any difference."""
import os
import re
import subprocess
import sys
import tempfile

SOURCES = ["attn_fwd.hip", "attn_fwd_fp8.hip", "attn_fwd_mx.hip", "attn_fwd_i8.hip"]
DESCRIPTOR = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def flags(tree):
    sys.path.insert(0, tree)
    from vorta_amd import build
    sys.path.pop(0)
    return [f for f in build.FLAGS if not f.startswith("-I")]


def key(mangled):
    name, targs, params = re.match(r"_ZN(?:12_GLOBAL__N_1|10vorta_attn)\d+(\w+?_kernel)I(.*?)EEv(.*)$", mangled).groups()
    if "combine" in name:  # output type (DF16b / DF16_) + parameter block
        return "attn_combine_kernel<%s,%s>" % (targs[:5], re.search(r"Params(8|Mx|I8)?", targs + params).group(0))
    return "%s<%s>" % (name, targs)


def kernels(tree, source, fl, out):
    csrc = os.path.join(tree, "vorta_amd", "csrc")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + fl + ["-I" + os.path.join(tree, "include"),
                          "-I" + csrc, "-S", "--cuda-device-only", os.path.join(csrc, source), "-o", out])
    text = open(out).read()
    res = {}
    for m in re.finditer(r"\n(_Z\S+):[^\n]*\n(.*?)\n\.Lfunc_end\d+:", text, re.S):
        body = re.sub(r"_Z[\w.]+", "SYM", re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", m.group(2)))
        res[m.group(1)] = ["\n".join(l.split(";")[0].rstrip() for l in body.split("\n") if l.split(";")[0].strip())]
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        res[m.group(1)].append({k: re.search(r"\.amdhsa_%s\s+(\S+)" % k, m.group(2)).group(1) for k in DESCRIPTOR})
    return {key(n): v for n, v in res.items()}


def main():
    old, new = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    fl, bad = flags(new), False
    with tempfile.TemporaryDirectory() as td:
        for source in sys.argv[3:] or SOURCES:
            a = kernels(old, source, fl, os.path.join(td, "old.s"))
            b = kernels(new, source, fl, os.path.join(td, "new.s"))
            diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
            bad |= bool(diff)
            print("%-18s %3d kernels: %s" % (source, len(b), "identical" if not diff else "DIFFERENT " + ", ".join(diff)))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
