#!/usr/bin/env python3
"""Did a change leave the device code as it was?  Takes two device assembly files (hipcc -S --cuda-device-only), or two
checkouts whose library it compiles for gfx950 as tools/isa_price.py does (no GPU needed), cuts both into functions by
symbol and compares them one by one.  What differs between two builds of the same code is taken out first: the numbers of
the block labels (.LBB<n>_, .Lfunc_end<n>, .LJTI<n>_) and the __hip_cuid_ symbol.

It prints how many functions are identical, and for every other one its symbol, the instruction counts by class (the
classes of isa_price.py), the registers, scratch and LDS of both sides and the compiler's occupancy comment.  It only
compares: it looks for nothing inside the code.

    python tools/isa_same.py before.s after.s
    python tools/isa_same.py ../parent-checkout .          # compiles both (about a minute each)

Exit status: 0 when every function is identical, 1 otherwise.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_price import price, resources  # noqa: E402

CLASSES = ("valu", "salu", "vmem", "lds", "other")
LABEL_NUMBERS = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI|LCPI)\d+")
CUID = re.compile(r"__hip_cuid_\w+")


def device_asm(root):
    src = os.path.join(root, "fastq_utils_amd", "csrc", "fqg_abi.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "device.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                        src, "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read()


def normalise(text):
    return CUID.sub("__hip_cuid_", LABEL_NUMBERS.sub(r".\1", text))


def functions(text):
    """{symbol: (body lines, the compiler's comments behind the body)} of every function of a listing"""
    out = {}
    for name in dict.fromkeys(re.findall(r"^\s*\.type\s+([\w$.]+),@function", text, re.M)):
        m = re.search(r"^" + re.escape(name) + r":.*?^\.Lfunc_end\d+:", text, re.M | re.S)
        if not m:
            continue
        after = text[m.end():]
        nxt = re.search(r"^\s*\.type\s+[\w$.]+,@function", after, re.M)
        body = [ln.rstrip() for ln in normalise(m.group(0)).splitlines() if ln.strip()]
        out[name] = (body, after[:nxt.start() if nxt else len(after)])
    return out


def class_counts(body):
    n = dict.fromkeys(CLASSES, 0)
    for ln in body[1:]:
        t = ln.strip()
        if t.startswith((";", ".")) or t.endswith(":") or re.match(r"[\w$.]+:", t):
            continue
        n[price(t)[0]] += 1
    return n


def figures(text, name, body, tail):
    """one line: instruction counts by class, registers, scratch, LDS, occupancy"""
    n = class_counts(body)
    res = resources(text, name)
    occ = re.search(r";\s*Occupancy:\s*(\d+)", tail)
    return (", ".join(f"{k} {n[k]}" for k in CLASSES) +
            f" | vgpr {res.get('vgpr_count', '-')}, sgpr {res.get('sgpr_count', '-')}, "
            f"scratch {res.get('private_segment_fixed_size', '-')}, lds {res.get('group_segment_fixed_size', '-')}, "
            f"occupancy {occ.group(1) if occ else '-'}")


def compare(text_a, text_b, out=sys.stdout):
    """prints the report; returns the symbols that are not identical"""
    fa, fb = functions(text_a), functions(text_b)
    names = list(dict.fromkeys(list(fa) + list(fb)))
    differ = [n for n in names if n not in fa or n not in fb or fa[n][0] != fb[n][0]]
    print(f"{len(names) - len(differ)} of {len(names)} device functions identical", file=out)
    for n in differ:
        print(f"== {n}", file=out)
        for side, text, fs in (("a", text_a, fa), ("b", text_b, fb)):
            print(f"   {side}: " + (figures(text, n, *fs[n]) if n in fs else "not there"), file=out)
    return differ


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a", help="device assembly file, or a checkout to compile")
    ap.add_argument("b", help="the same for the other side")
    a = ap.parse_args()
    texts = [device_asm(p) if os.path.isdir(p) else open(p).read() for p in (a.a, a.b)]
    sys.exit(1 if compare(*texts) else 0)


if __name__ == "__main__":
    main()
