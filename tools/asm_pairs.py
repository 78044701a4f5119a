#!/usr/bin/env python3
"""Pair the kernels of two device-assembly files of csrc/conv_fwd.hip (``hipcc --cuda-device-only -S``, the build's flags) by
(kernel, form, arithmetic, mode) and compare each pair's instruction stream and its ``.amdhsa_`` resource block.

  tools/asm_pairs.py parent.s result.s > profiles/<name>.txt        (exit status 1 when a pair differs or has no partner)

The plain convolution's mode is a template argument: ``conv2d_fwd_kernel<F, S, BN>`` (mode 1 + BN) in trees before the mode
became ``FwdMode``, ``conv2d_fwd_kernel<F, S, (pleas::FwdMode)M>`` since.  Inside a body the kernel's own symbol and the
function index of its block labels are masked; nothing else is."""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.S | re.M):
        sym, res = m.group(1), m.group(2)
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(sym), text, re.S | re.M).group(1)
        mask = lambda t: re.sub(r"\.LBB\d+_", ".LBB_", t.replace(sym, "KERNEL"))
        out[sym] = (mask(body), mask(res))
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")
    keyed = {}
    for sym, name in zip(out, names):
        m = re.match(r"void pleas::(\w+)<(\d+), (\d+)(?:, (?:\(pleas::FwdMode\))?(\d+))?>", name)
        if m is None:
            key = (re.sub(r"\(.*", "", name).replace("pleas::", ""),)
        elif m.group(1) == "conv2d_fwd_kernel":
            key = (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)) + (0 if "FwdMode" in name else 1))
        else:
            key = (m.group(1), int(m.group(2)), int(m.group(3)), 0)
        assert key not in keyed, key
        keyed[key] = out[sym]
    return keyed


def resources(res):
    want = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")
    return " ".join("%s=%s" % (k, re.search(r"\.amdhsa_%s (\S+)" % k, res).group(1)) for k in want)


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    print("# kernel form arithmetic mode | instructions (lines) | resource block | registers / scratch / LDS")
    for key in sorted(set(a) | set(b), key=str):
        if key not in a or key not in b:
            print(*key, "| ONLY IN", "first" if key in a else "second")
            bad += 1
            continue
        same_body, same_res = a[key][0] == b[key][0], a[key][1] == b[key][1]
        bad += not (same_body and same_res)
        print(*key, "|", "identical" if same_body else "DIFFERENT", "(%d)" % a[key][0].count("\n"), "|",
              "identical" if same_res else "DIFFERENT", "|", resources(b[key][1]))
    print("# %d kernels in the first file, %d in the second, %d paired, %d differ or lack a partner"
          % (len(a), len(b), len(set(a) & set(b)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
