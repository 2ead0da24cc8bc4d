#!/usr/bin/env python3
"""isa_compare.py -- compare the device code of two `hipcc -S --cuda-device-only` outputs of csrc/dvo_kernels.hip kernel by kernel.

For every kernel of BEFORE: identical instruction stream / identical up to SGPR numbering / different, with (VGPRs, SGPRs, scratch
bytes, kernarg bytes) before and after.  --rename OLD=NEW pairs a kernel whose mangled name changed (e.g. a template parameter was
added); with --offsets, kernarg offsets are ignored too (a field added to an argument block moves the blocks after it).

    hipcc <Makefile FLAGS> -S --cuda-device-only -o before.s csrc/dvo_kernels.hip   (parent tree)
    hipcc <Makefile FLAGS> -S --cuda-device-only -o after.s  csrc/dvo_kernels.hip   (this tree)
    python tools/isa_compare.py before.s after.s [--only k_track_gn]
"""
import argparse
import re


def kernels(path):
    txt = open(path).read()
    body = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):\s*;.*?\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M)}
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        g = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, m.group(2)).group(1))
        meta[m.group(1)] = (g("next_free_vgpr"), g("next_free_sgpr"), g("private_segment_fixed_size"))
    return body, meta


def norm(body, sgpr=False, offsets=False):
    lines = [l.split(";")[0].rstrip() for l in body.split("\n")]
    s = "\n".join(re.sub(r"\.LBB\d+_", ".LBB_", l) for l in lines if l.strip() and not l.strip().startswith("."))
    if sgpr:
        s = re.sub(r"\bs\[\d+:\d+\]", "s[]", s)
        s = re.sub(r"\bs\d+\b", "sN", s)
    if offsets:
        s = re.sub(r"0x[0-9a-f]+", "IMM", s)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before"); ap.add_argument("after")
    ap.add_argument("--only", default="", help="substring a kernel name must contain")
    ap.add_argument("--rename", action="append", default=[], help="OLD=NEW mangled names")
    ap.add_argument("--offsets", action="store_true", help="also ignore immediate offsets (kernarg layout)")
    a = ap.parse_args()
    b0, m0 = kernels(a.before)
    b1, m1 = kernels(a.after)
    ren = dict(r.split("=", 1) for r in a.rename)
    for name in sorted(b0):
        if a.only not in name:
            continue
        new = ren.get(name, name)
        if new not in b1:
            print("%-64s gone" % name[:64])
            continue
        if norm(b0[name]) == norm(b1[new]):
            verdict = "identical"
        elif norm(b0[name], True) == norm(b1[new], True):
            verdict = "identical up to SGPR numbering"
        elif a.offsets and norm(b0[name], True, True) == norm(b1[new], True, True):
            verdict = "identical up to SGPR numbering and offsets"
        else:
            verdict = "DIFFERENT"
        print("%-64s %5d instructions  %-44s %s -> %s" % (new[:64], len(norm(b1[new]).split("\n")), verdict, m0.get(name), m1.get(new)))
    added = [n for n in b1 if n not in b0 and n not in ren.values() and a.only in n]
    for n in sorted(added):
        print("%-64s new  (VGPRs, SGPRs, scratch) %s" % (n[:64], m1.get(n)))


if __name__ == "__main__":
    main()
