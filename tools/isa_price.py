#!/usr/bin/env python3
"""What do a kernel's vector instructions cost?  Compiles the library's device code for gfx950 (no GPU needed; or takes
an assembly file made before), cuts one kernel out, splits it into basic blocks and prices the vector-ALU instructions of
every block by the list of profiles/ANALYSIS_r04.md (tools/kbench/valubench.hip, cycles of a SIMD per wavefront):

    2.3   v_and / or / xor / not / mov_b32, v_add / sub / subrev_u32, v_lshrrev_b32, v_ashrrev_i32 on registers, a
          literal or an inline constant; v_bitop3_b32 on three registers
    4.4   every other vector-ALU instruction, and any of the above that reads an SGPR (vcc, exec and m0 included) or has
          a DPP or SDWA form

The list has no price of its own for 64-bit and double-precision forms: they take the 4.4 of "every other", which is a
floor for them.  Memory, LDS and scalar instructions are counted, not priced.  A static count: how often a block runs
is for the reader to say - name the blocks of the path that matters with --path and their prices are added up.

    python tools/isa_price.py k_stream_lines_fast
    python tools/isa_price.py k_stream_lines_fast --asm device.s --path LBB11_15,bb.16,LBB11_21
    python tools/isa_price.py k_stream_pass1ILj0ELi0E --totals      # one line per kernel, no block table
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHEAP, DEAR = 2.3, 4.4
CHEAP_OPS = {"v_and_b32", "v_or_b32", "v_xor_b32", "v_not_b32", "v_mov_b32", "v_add_u32", "v_sub_u32", "v_subrev_u32",
             "v_lshrrev_b32", "v_ashrrev_i32", "v_bitop3_b32"}
FREE_OPS = {"v_nop"}
SCALAR_OPERAND = re.compile(r"(?<![\w.])(s\d+|s\[\d+:\d+\]|vcc(_lo|_hi)?|exec(_lo|_hi)?|m0|scc)(?![\w])")
DPP_SDWA = re.compile(r"\b(quad_perm|row_shl|row_shr|row_ror|row_bcast|row_mirror|row_half_mirror|wave_shl|wave_shr|"
                      r"wave_rol|wave_ror|row_newbcast|dst_sel|src0_sel|src1_sel|dpp8)\b")


def device_asm():
    src = os.path.join(REPO, "fastq_utils_amd", "csrc", "fqg_abi.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "device.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                        src, "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read()


def price(line):
    """(kind, cycles) of one instruction line; kind: valu, salu, vmem, lds, other"""
    t = line.split(";")[0].strip()
    op = t.split()[0]
    base = re.sub(r"_(e32|e64|dpp|sdwa|e64_dpp)$", "", op)
    if op.startswith("v_"):
        if base in FREE_OPS:
            return "valu", 0.0
        dear = base not in CHEAP_OPS or op.endswith(("_dpp", "_sdwa")) or DPP_SDWA.search(t) or \
            SCALAR_OPERAND.search(t[len(op):])
        return "valu", DEAR if dear else CHEAP
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem", 0.0
    if op.startswith("ds_"):
        return "lds", 0.0
    if op.startswith("s_"):
        return "salu", 0.0
    return "other", 0.0


def blocks_of(body):
    """[(name, loop note, [instruction lines])] in program order"""
    out, cur = [], ("entry", "", [])
    for line in body.splitlines()[1:]:
        t = line.strip()
        m = re.match(r"(\.LBB\d+_\d+):|; %(bb\.\d+):", t)
        if m:
            if cur[2] or cur[0] == "entry":
                out.append(cur)
            note = re.search(r"(=>This .*|in Loop: .*|Parent Loop .*)$", t)
            cur = ((m.group(1) or m.group(2)).lstrip("."), note.group(1).strip() if note else "", [])
            continue
        if not t or t.startswith((";", ".")):
            continue
        cur[2].append(t)
    out.append(cur)
    return out


def resources(text, name):
    at = text.find(".name:           " + name + "\n")
    meta = ""
    if at >= 0:  # the kernel's entry of amdhsa.kernels: from the "  - ." in front of its name to the next one
        end = text.find("\n  - .", at)
        meta = text[text.rfind("\n  - .", 0, at):end if end >= 0 else len(text)]
    keys = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
            "group_segment_fixed_size")
    got = {}
    for k in keys:
        m = re.search(r"\." + k + r":\s+(\d+)", meta)
        if m:
            got[k] = int(m.group(1))
    return got


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernel", help="fragment of the mangled name")
    ap.add_argument("--asm", help="device assembly made before (hipcc -S --cuda-device-only) instead of compiling now")
    ap.add_argument("--path", default="", help="comma-separated block names whose prices are added up")
    ap.add_argument("--totals", action="store_true", help="one line per kernel only")
    a = ap.parse_args()
    text = open(a.asm).read() if a.asm else device_asm()
    names = [m.group(1) for m in re.finditer(r"^(_Z\w+):", text, re.M) if a.kernel in m.group(1)]
    if not names:
        sys.exit(f"no kernel matches {a.kernel!r}")
    path = [p.strip().lstrip(".") for p in a.path.split(",") if p.strip()]
    for name in names:
        body = text[text.index(f"\n{name}:") + 1:]
        body = body[:body.index(".Lfunc_end")]
        blocks = blocks_of(body)
        res = resources(text, name)
        print(f"== {name}")
        print("   " + ", ".join(f"{k} {v}" for k, v in res.items()))
        tot = {"valu": 0, "salu": 0, "vmem": 0, "lds": 0, "other": 0}
        tot_cyc, rows, on_path = 0.0, [], {}
        for bname, note, lines in blocks:
            n = {"valu": 0, "salu": 0, "vmem": 0, "lds": 0, "other": 0}
            cyc = 0.0
            for ln in lines:
                kind, c = price(ln)
                n[kind] += 1
                cyc += c
            for k in n:
                tot[k] += n[k]
            tot_cyc += cyc
            rows.append((bname, n, cyc, note))
            if bname in path:
                on_path[bname] = (n, cyc)
        if not a.totals:
            print(f"   {'block':<12}{'valu':>6}{'cycles':>9}{'salu':>6}{'vmem':>6}{'lds':>5}  loop")
            for bname, n, cyc, note in rows:
                mark = "*" if bname in path else " "
                print(f"  {mark}{bname:<12}{n['valu']:>6}{cyc:>9.1f}{n['salu']:>6}{n['vmem']:>6}{n['lds']:>5}  {note}")
        print(f"   whole kernel (static): valu {tot['valu']}, priced {tot_cyc:.1f} cycles, salu {tot['salu']}, "
              f"vmem {tot['vmem']}, lds {tot['lds']}")
        if path:
            missing = [p for p in path if p not in on_path]
            if missing:
                sys.exit(f"no such block: {missing}")
            nv = sum(on_path[p][0]["valu"] for p in path)
            ns = sum(on_path[p][0]["salu"] for p in path)
            nm = sum(on_path[p][0]["vmem"] for p in path)
            nl = sum(on_path[p][0]["lds"] for p in path)
            print(f"   path ({len(path)} blocks): valu {nv}, priced {sum(on_path[p][1] for p in path):.1f} cycles, "
                  f"salu {ns}, vmem {nm}, lds {nl}")
        print()


if __name__ == "__main__":
    main()
