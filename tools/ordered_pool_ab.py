#!/usr/bin/env python3
"""The two programs whose loops over several contexts hand their results over through host/fq_ordered.h, this tree's
against another build's (the parent commit's): `fastq_info -r` and `fastq_pre_barcodes --sam` with FQGPU_DEVICES=0,0 on
plain files of about 1 GiB on tmpfs, output to /dev/null, builds alternating, `seconds` of FQGPU_JSON_METRICS.  One more
run per build, not timed, keeps stdout and stderr: they must be the same.
usage: tools/ordered_pool_ab.py <directory with the other build's fastq_info and fastq_pre_barcodes> [million reads]; REPS=<runs per build>"""
import filecmp, json, os, shutil, statistics, subprocess, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAR = os.path.abspath(sys.argv[1])
N = float(sys.argv[2]) if len(sys.argv) > 2 else 3.4
REPS = int(os.environ.get("REPS", 5))
D = "/dev/shm/fqg_ordered_ab"; os.makedirs(D, exist_ok=True)
def say(s):
    print(s, flush=True)
def write(path, n, read_len, seed, qlo=35):
    rng = np.random.default_rng(seed)
    with open(path, "wb") as f:
        done = 0
        while done < n:
            m = min(1_000_000, n - done); w = 12 + 1 + read_len + 1 + 2 + read_len + 1
            rec = np.empty((m, w), dtype=np.uint8)
            names = np.char.zfill(np.arange(done, done + m).astype("U"), 10)
            rec[:, 0] = ord("@"); rec[:, 1] = ord("r")
            rec[:, 2:12] = np.frombuffer("".join(names).encode(), dtype=np.uint8).reshape(m, 10)
            rec[:, 12] = 10; rec[:, 13:13 + read_len] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), (m, read_len))
            rec[:, 13 + read_len] = 10; rec[:, 14 + read_len] = ord("+"); rec[:, 15 + read_len] = 10
            rec[:, 16 + read_len:16 + 2 * read_len] = rng.integers(qlo, 74, (m, read_len), dtype=np.uint8); rec[:, 16 + 2 * read_len] = 10
            f.write(rec.tobytes()); done += m
n = int(N * 1_000_000)
write(f"{D}/a_1.fastq", n, 150, 1)
write(f"{D}/i1.fastq", n, 26, 3, qlo=40)   # (a few index reads fall below --min_qual 10 + 33: the discards)
V2 = ["--read1", "a_1.fastq", "--index1", "i1.fastq", "--umi_read", "index1", "--umi_offset", "16", "--umi_size", "10",
      "--cell_read", "index1", "--cell_offset", "0", "--cell_size", "16", "--phred_encoding", "33", "--min_qual", "10"]
LEGS = [("fastq_info -r", ["fastq_info", "-r", "a_1.fastq"]),
        ("fastq_pre_barcodes --sam", ["fastq_pre_barcodes"] + V2 + ["--sam", "--outfile1", "-"])]
say(f"{n} reads of 150 bp ({os.path.getsize(D + '/a_1.fastq') >> 20} MiB) and their 26 bp index reads, plain, on tmpfs; FQGPU_DEVICES=0,0; "
    f"{REPS} runs per build, parent / new alternating; `seconds` of FQGPU_JSON_METRICS")
# (the other build's programs find the library of this tree: the library is the same in both)
env0 = dict(os.environ, FQGPU_DEVICES="0,0", LD_LIBRARY_PATH=os.path.join(REPO, "fastq_utils_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
bad = 0
for label, cmd in LEGS:
    exe = {"parent": os.path.join(PAR, cmd[0]), "new": os.path.join(REPO, "bin", cmd[0])}
    secs = {"parent": [], "new": []}
    for rep in range(REPS + 1):
        for b in ("parent", "new"):
            last = rep == REPS  # the run that is kept, not timed
            jm = f"{D}/metrics.json"
            with open(f"{D}/out_{b}" if last else os.devnull, "wb") as out:
                p = subprocess.run(cmd, executable=exe[b], cwd=D, stdout=out, stderr=subprocess.PIPE, env=dict(env0, FQGPU_JSON_METRICS=jm), timeout=300)
            if p.returncode:
                say(f"!! {label} {b} exit {p.returncode} {p.stderr[-300:]}"); sys.exit(1)
            if last:
                open(f"{D}/err_{b}", "wb").write(p.stderr)
            else:
                secs[b].append(json.load(open(jm))["seconds"])
            os.remove(jm)
    pm, nm = statistics.median(secs["parent"]), statistics.median(secs["new"])
    ok = nm <= max(secs["parent"]); bad += not ok   # (below the parent's fastest run is no finding)
    same = filecmp.cmp(f"{D}/out_parent", f"{D}/out_new", False) and filecmp.cmp(f"{D}/err_parent", f"{D}/err_new", False)
    bad += not same
    say(f"{label:26s} parent median {pm:6.3f} (min {min(secs['parent']):6.3f} max {max(secs['parent']):6.3f})  new median {nm:6.3f} (min {min(secs['new']):6.3f} max {max(secs['new']):6.3f})  "
        f"new median {'not above' if ok else 'ABOVE'} the parent's range; stdout ({os.path.getsize(D + '/out_new')} bytes) and stderr {'same' if same else 'DIFFERENT'}")
    say(f"      parent {[round(x, 3) for x in secs['parent']]}  new {[round(x, 3) for x in secs['new']]}")
say(f"findings: {bad}")
shutil.rmtree(D)
sys.exit(1 if bad else 0)
