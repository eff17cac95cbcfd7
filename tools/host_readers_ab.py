#!/usr/bin/env python3
"""Host-only cost of the three staging classes (host/fq_input.h, fq_multi.h, fq_blocks.h) on this tree against another
checkout of the repository: their test drivers (tests/cxx/input_sanitize.cpp, pieces_check.cpp, blocks_check.cpp; pinned
allocation = malloc, no GPU) built -O2 from both trees, run alternating over one file of N million 150 bp reads on tmpfs,
plain and gzip -1, with what FQGPU_TIMING says in an extra run.
usage: tools/host_readers_ab.py <other checkout> [million reads]; REPS=<runs per build> ONLY=<part of a leg's name> SFX=<''|.gz>"""
import gzip, os, shutil, statistics, subprocess, sys, time
import numpy as np
NEW, PAR = os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.abspath(sys.argv[1])
D = "/dev/shm/fqg_host_ab"; os.makedirs(D, exist_ok=True)
def say(s):
    print(s, flush=True)
N = int(sys.argv[2]) if len(sys.argv) > 2 else 3
REPS = int(os.environ.get("REPS", 4))
exes = {}
for b, root in (("parent", PAR), ("new", NEW)):
    for drv in ("input_sanitize", "pieces_check", "blocks_check"):
        exe = f"{D}/{drv}_{b}"
        subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-o", exe, f"{root}/tests/cxx/{drv}.cpp", "-lz"], check=True)
        exes[(drv, b)] = exe
rng = np.random.default_rng(1)
n, L = N * 1_000_000, 150
with open(f"{D}/a.fastq", "wb") as f:
    done = 0
    while done < n:
        m = min(1_000_000, n - done); w = 12 + 1 + L + 1 + 2 + L + 1
        rec = np.empty((m, w), dtype=np.uint8)
        names = np.char.zfill(np.arange(done, done + m).astype("U"), 10)
        rec[:, 0] = ord("@"); rec[:, 1] = ord("r")
        rec[:, 2:12] = np.frombuffer("".join(names).encode(), dtype=np.uint8).reshape(m, 10)
        rec[:, 12] = 10; rec[:, 13:13 + L] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), (m, L))
        rec[:, 13 + L] = 10; rec[:, 14 + L] = ord("+"); rec[:, 15 + L] = 10
        rec[:, 16 + L:16 + 2 * L] = rng.integers(35, 74, (m, L), dtype=np.uint8); rec[:, 16 + 2 * L] = 10
        f.write(rec.tobytes()); done += m
with open(f"{D}/a.fastq", "rb") as i, gzip.open(f"{D}/a.fastq.gz", "wb", compresslevel=1) as o:
    shutil.copyfileobj(i, o, 1 << 24)
say(f"{N} M reads of 150 bp on tmpfs ({os.path.getsize(D + '/a.fastq') >> 20} MiB plain, {os.path.getsize(D + '/a.fastq.gz') >> 20} MiB gzip -1); test drivers built -O2, pinned allocation = malloc, no GPU; "
    f"{REPS} runs per build, parent / new alternating, seconds of wall time (the drivers' own checking of every byte included, the same in both)")
LEGS = [("Input, pieces of 64 MiB", "input_sanitize", ["67108864", "0"]),
        ("Input, whole file", "input_sanitize", ["67108864", "2"]),
        ("AlignedPieces 64 MiB, 3 consumers", "pieces_check", ["67108864", "3"]),
        ("RecordBlocks 200000 records, 3 consumers", "blocks_check", ["200000", "3"])]
bad = 0
for sfx in ("", ".gz"):
    for label, drv, args in [l for l in LEGS if os.environ.get("ONLY", "") in l[0] and os.environ.get("SFX", sfx) == sfx]:
        times = {"parent": [], "new": []}; says = {}; outs = {}
        for rep in range(REPS + 1):
            for b in ("parent", "new"):
                env = dict(os.environ, FQGPU_TIMING="1") if rep == REPS else dict(os.environ)
                t0 = time.perf_counter()
                p = subprocess.run([exes[(drv, b)], f"{D}/a.fastq{sfx}"] + args, capture_output=True, env=env, timeout=600)
                dt = time.perf_counter() - t0
                if p.returncode: say(f"!! {label} {b} exit {p.returncode} {p.stdout} {p.stderr[-300:]}"); sys.exit(1)
                outs[b] = p.stdout.strip()
                if rep < REPS: times[b].append(dt)
                else: says[b] = [l[l.find("fqgpu timing"):] for l in p.stderr.decode("latin-1").splitlines() if "fqgpu timing" in l]
        pm, nm = statistics.median(times["parent"]), statistics.median(times["new"]); spread = max(times["parent"]) - min(times["parent"])
        ok = abs(nm - pm) <= spread; bad += not ok
        say(f"{label:42s} {'gz   ' if sfx else 'plain'} parent median {pm:6.3f} (min {min(times['parent']):6.3f} max {max(times['parent']):6.3f} spread {spread:5.3f})  new median {nm:6.3f} (min {min(times['new']):6.3f} max {max(times['new']):6.3f})  "
            f"new - parent {nm - pm:+6.3f}  {'within' if ok else 'OUTSIDE'} the parent's spread; output {'same' if outs['parent'] == outs['new'] else 'DIFFERENT'}")
        say(f"      parent {[round(x, 3) for x in times['parent']]}  new {[round(x, 3) for x in times['new']]}")
        for b in ("parent", "new"):
            for s in says[b]: say(f"      [{b}] " + s[:330])
say(f"legs outside the parent's spread: {bad}")
shutil.rmtree(D)
