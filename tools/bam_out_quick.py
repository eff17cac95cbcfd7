"""fastq_pre_barcodes --bam against --sam on one box: python tools/bam_out_quick.py [million pairs [bin]]

Input: synthetic pairs in the 10x v2 layout (index1 = 16 bp cell barcode + 10 bp UMI, read1 = 150 bp cDNA, the flags
sh/fastq2bam:125-130 builds plus --phred_encoding 33 --min_qual 10), two plain files.

  kernels   the emit and plan kernels' time (fqg_profile_read) of fqg_barcodes_transform on the same reads, resident on
            the device, for SAM lines and for BAM records, and the bytes each leaves on the device  [this tree's library]
  programs  wall time, three runs each and their median, and the bytes written, of
              --sam > file                      (what the reference's pipeline hands to samtools view -b)
              --bam > file                      (the host's threads compress)
              --bam > file, FQGPU_GZIP_GPU=1    (the device compresses)
              FASTQ mode (--outfile1 o.fastq.gz)
            `bin`: the folder of the programs (default: this tree's).  The parent commit's has no --bam: its --sam and
            FASTQ legs, in the same session, are what this tree's are held against.

The pipeline's `samtools view -b` leg is not timed (no samtools here): the comparison is --bam's wall time against
--sam's wall time alone.  One JSON document on stdout; nothing is asserted."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import fastq_utils_amd as fq  # noqa: E402

A = fq.abi
pairs = int(float(sys.argv[1]) * 1e6) if len(sys.argv) > 1 else 2_000_000
BIN = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(REPO, "bin")
RUNS = 3
out = {"pairs": pairs, "runs": RUNS, "bin": os.path.relpath(BIN, REPO), "kernels": {}, "programs": {}}

with tempfile.TemporaryDirectory() as tmp:
    paths = {"i1": os.path.join(tmp, "i1.fastq"), "r1": os.path.join(tmp, "r1.fastq")}
    with fq.Context(0) as ctx:
        R1, R2 = A.synth_record_bytes(26), A.synth_record_bytes(150)
        img1 = torch.empty(pairs * R1, dtype=torch.uint8, device="cuda:0")
        img2 = torch.empty(pairs * R2, dtype=torch.uint8, device="cuda:0")
        ctx.synth_fastq(img1.data_ptr(), pairs, 26, first_index=0, seed=777, mate=1)
        ctx.synth_fastq(img2.data_ptr(), pairs, 150, first_index=0, seed=778, mate=2)
        ctx.synchronize()
        # barcode qualities: Phred 12 and more, one base below Phred 10 in about 5 % of the reads (they are discarded)
        q = img1.view(pairs, R1)[:, 45 + 26 + 3: 45 + 26 + 3 + 26]
        q.clamp_(min=33 + 12)
        g = torch.Generator(device="cuda:0")
        g.manual_seed(99)
        rows = torch.nonzero(torch.rand(pairs, generator=g, device="cuda:0") < 0.05).squeeze(1)
        q[rows, torch.randint(0, 26, (rows.numel(),), generator=g, device="cuda:0")] = 33 + 5
        torch.cuda.synchronize()
        st1 = A.probe_first_record(bytes(img1[: 4 * R1].cpu().numpy()), True)
        st2 = A.probe_first_record(bytes(img2[: 4 * R2].cpu().numpy()), True)
        if BIN == os.path.join(REPO, "bin"):   # (the library under this script is this tree's, whatever `bin` is)
            frames, states = {}, {A.READ1: st2, A.INDEX1: st1}
            for key, img, st, R in ((A.READ1, img2, st2, R2), (A.INDEX1, img1, st1, R1)):
                r = ctx.validate(img.data_ptr(), None, st, final=True, flags=A.VALIDATE_FRAME_ONLY, nbytes=pairs * R)
                assert r["n_records"] == pairs, r
                frames[key] = ctx.retain_frame()
            for kind, sam in (("sam", A.OUT_SAM), ("bam", A.OUT_BAM)):
                runs = []
                for rep in range(RUNS + 1):
                    ctx.profile(True)
                    ctx.profile_reset()
                    r = ctx.barcodes_transform(frames, states, pairs, umi=(A.INDEX1, 16, 10), cell=(A.INDEX1, 0, 16), phred=33, min_qual=10, sam=sam)
                    ctx.synchronize()
                    prof = {k: round(v[1], 3) for k, v in ctx.profile_read().items() if k.startswith("k_bc") and v[0] > 0}
                    ctx.profile(False)
                    assert r["code"] == 0 and r["n_done"] == pairs, r
                    if rep:
                        runs.append(prof)
                out["kernels"][kind] = {"out_bytes": r["out_bytes"][0], "kept": pairs - r["n_discarded"], "runs_ms": runs,
                                        "median_ms": {k: statistics.median(p[k] for p in runs) for k in runs[0]}}
            for f in frames.values():
                f.release()
        for key, img in (("i1", img1), ("r1", img2)):
            with open(paths[key], "wb") as f:
                f.write(bytes(img.cpu().numpy()))
        out["input_bytes"] = pairs * (R1 + R2)
        del img1, img2, q
    v2 = ["--read1", paths["r1"], "--index1", paths["i1"], "--umi_read", "index1", "--umi_offset", "16", "--umi_size", "10", "--cell_read", "index1",
          "--cell_offset", "0", "--cell_size", "16", "--phred_encoding", "33", "--min_qual", "10"]
    # (does this build know --bam?  One that does not ignores the word and writes a gzip'd FASTQ file to stdout: no BGZF field)
    tiny = os.path.join(tmp, "tiny.fastq")
    with open(tiny, "wb") as f:
        f.write(b"@r 1:N:0\nACGT\n+\nIIII\n")
    probe = subprocess.run([os.path.join(BIN, "fastq_pre_barcodes"), "--read1", tiny, "--bam", "--outfile1", "-"], capture_output=True)
    has_bam = probe.returncode == 0 and probe.stdout[12:14] == b"BC"
    legs = [("--sam > file", v2 + ["--sam", "--outfile1", "-"], {}),
            ("FASTQ mode", v2 + ["--outfile1", os.path.join(tmp, "o.fastq.gz")], {})]
    if has_bam:
        legs += [("--bam > file (host compressor)", v2 + ["--bam", "--outfile1", "-"], {}),
                 ("--bam > file (FQGPU_GZIP_GPU=1)", v2 + ["--bam", "--outfile1", "-"], {"FQGPU_GZIP_GPU": "1"})]
    for leg, args, env in legs:
        e = dict(os.environ)
        for k in ("FQGPU_GZIP_GPU", "FQGPU_GZIP_FAST", "FQGPU_GZIP_LEVEL", "FQGPU_SERIAL_LOOP", "FQGPU_DEVICES"):
            e.pop(k, None)
        e.update(env)
        wall, size = [], 0
        for rep in range(RUNS):
            target = os.path.join(tmp, "stdout")
            with open(target, "wb") as so:
                t0 = time.perf_counter()
                p = subprocess.run([os.path.join(BIN, "fastq_pre_barcodes")] + args, env=e, stdout=so, stderr=subprocess.PIPE)
                wall.append(time.perf_counter() - t0)
            assert p.returncode == 0, p.stderr[-400:]
            size = os.path.getsize(target) + (os.path.getsize(os.path.join(tmp, "o.fastq.gz")) if leg == "FASTQ mode" else 0)
        out["programs"][leg] = {"wall_s": [round(w, 3) for w in wall], "median_wall_s": round(statistics.median(wall), 3),
                                "spread_s": round(max(wall) - min(wall), 3), "bytes_written": size}
print(json.dumps(out, indent=1))
