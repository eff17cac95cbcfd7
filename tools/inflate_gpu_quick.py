"""The device inflater (fqg_bgzf_inflate, FQGPU_INFLATE_GPU=1) on one box: python tools/inflate_gpu_quick.py [runs [bin]]

  files     reads_500k: an unaligned BAM of 500 000 synthetic 150-base reads as tools/gzip_gpu_quick.py makes it (random
            bases and qualities: 0.3 of its size compressed); tagged_500k: 500 000 alignments of tests/bamgen.py's config4
            (124 bytes each, CR / GX / RX tags, what bam_umi_count reads: 0.08 compressed); tagged_1k: its first 1 000 as a
            file of its own (a few blocks: the device is not filled); tests/golden/data_b2f/test10e6.bam.  BGZF blocks of
            0xff00 bytes by zlib level 6, as samtools writes them
  kernel    GB/s of INFLATED bytes through k_inflate_blocks (fqg_profile_read)
  call      fqg_bgzf_inflate + fqg_inflate_output against fqhost::bgzf_inflate_parallel on the same bytes in the same
            process (tools/inflate_call_bench.cpp), wall time
  programs  bin/bam2fastq and bin/bam_add_tags on reads_500k, bin/bam_umi_count on tagged_500k, all three on tagged_1k: wall
            time, default and FQGPU_INFLATE_GPU=1.  `bin`: the
            folder of the programs (default: this tree's), to run another build of them - the parent commit's, which
            knows the default mode only - through the same legs in the same session

Every figure with its individual runs beside the median.  One JSON document on stdout.  Nothing is asserted about speed:
the numbers go to profiles/."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

from tests import bamgen  # noqa: E402

RUNS = max(3, int(sys.argv[1])) if len(sys.argv) > 1 else 5
BIN = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(REPO, "bin")
OURS = BIN == os.path.join(REPO, "bin")


def bam_of(text, n, R):
    """an unaligned BAM stream of the first n synthetic records (R bytes each, 150 bases): the names as
    fastq_pre_barcodes writes them (STAGS_CELL=.._UMI=.._SAMPLE=.._ETAGS_<name>), the reads' bases and qualities"""
    L = 150
    a = np.frombuffer(text, dtype=np.uint8, count=n * R).reshape(n, R)
    rng = np.random.default_rng(1)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    name = a[:, 1:R - (2 * L + 5)].copy()
    name[name == 32] = 95
    parts = [np.broadcast_to(np.frombuffer(b"STAGS_CELL=", dtype=np.uint8), (n, 11)), acgt[rng.integers(0, 4, (n, 16))],
             np.broadcast_to(np.frombuffer(b"_UMI=", dtype=np.uint8), (n, 5)), acgt[rng.integers(0, 4, (n, 10))],
             np.broadcast_to(np.frombuffer(b"_SAMPLE=", dtype=np.uint8), (n, 8)), acgt[rng.integers(0, 4, (n, 8))],
             np.broadcast_to(np.frombuffer(b"_ETAGS_", dtype=np.uint8), (n, 7)), name, np.zeros((n, 1), dtype=np.uint8)]
    qname = np.concatenate(parts, axis=1)
    code = np.full(256, 15, dtype=np.uint8)
    for ch, v in zip(b"ACGT", (1, 2, 4, 8)):
        code[ch] = v
    nib = code[a[:, R - (2 * L + 4):R - (L + 4)]]
    seq = (nib[:, 0::2] << 4) | nib[:, 1::2]
    qual = a[:, R - (L + 1):R - 1] - 33
    body = 32 + qname.shape[1] + 4 + L // 2 + L
    core = np.zeros((n, 36), dtype=np.uint8)
    core[:, 0:4] = np.frombuffer(np.uint32(body).tobytes(), dtype=np.uint8)
    core[:, 4:8] = 255                                                 # refID -1
    core[:, 8:12] = 255                                                # pos -1
    core[:, 12] = qname.shape[1]                                       # l_read_name, mapq 0
    core[:, 14:16] = np.frombuffer(np.uint16(4680).tobytes(), dtype=np.uint8)  # bin
    core[:, 16] = 1                                                    # one CIGAR operation
    core[:, 18] = 4                                                    # flag: unmapped
    core[:, 20:24] = np.frombuffer(np.uint32(L).tobytes(), dtype=np.uint8)
    core[:, 24:32] = 255                                               # mate refID, mate pos -1
    cigar = np.broadcast_to(np.frombuffer(np.uint32(L << 4).tobytes(), dtype=np.uint8), (n, 4))
    recs = np.concatenate([core, qname, cigar, seq, qual], axis=1)
    head = b"@HD\tVN:1.0\tSO:unsorted\n"
    return b"BAM\x01" + len(head).to_bytes(4, "little") + head + (0).to_bytes(4, "little") + recs.tobytes()


def med(xs):
    return round(statistics.median(xs), 3)


out = {"runs": RUNS, "bin": os.path.relpath(BIN, REPO), "cpus_in_affinity_mask": len(os.sched_getaffinity(0)), "files": {}, "programs": {}}
with tempfile.TemporaryDirectory() as tmp:
    import torch

    import fastq_utils_amd as fq
    with fq.Context(0) as ctx:
        R = fq.abi.synth_record_bytes(150)
        img = torch.empty(500000 * R + 64, dtype=torch.uint8, device="cuda:0")
        ctx.synth_fastq(img.data_ptr(), 500000, 150)
        ctx.synchronize()
        reads = bam_of(bytes(img[:500000 * R].cpu().numpy()), 500000, R)
        del img
    rec, _, _, _ = bamgen.config4(np.random.default_rng(4), n_cells=2000, n_genes=5000, n_triples=385000)
    rec = rec[:500000]
    files = {}
    for name, stream in (("reads_500k", reads), ("tagged_500k", bamgen.header() + rec.tobytes()), ("tagged_1k", bamgen.header() + rec[:1000].tobytes())):
        files[name] = os.path.join(tmp, name + ".bam")
        with open(files[name], "wb") as f:
            f.write(bamgen.bgzf(stream))
    del reads
    golden = os.path.join(REPO, "tests", "golden", "data_b2f", "test10e6.bam")
    if os.path.exists(golden):
        files["golden_test10e6"] = golden
    if OURS:
        exe = os.path.join(tmp, "inflate_call_bench")
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(REPO, "tools", "inflate_call_bench.cpp"),
                        "-L" + os.path.join(REPO, "fastq_utils_amd"), "-lfqgpu", "-lz", "-pthread",
                        "-Wl,-rpath," + os.path.join(REPO, "fastq_utils_amd"), "-Wl,-rpath,/opt/rocm/lib"], check=True)
        for name, path in files.items():
            p = subprocess.run([exe, path, str(RUNS)], capture_output=True, text=True)
            assert p.returncode == 0, (name, p.returncode, p.stderr[-400:])
            r = json.loads(p.stdout)
            k, call, host = med(r["k_inflate_blocks_ms"]), med(r["device_call_ms"]), med(r["host_inflate_ms"])
            r.update({"median_k_inflate_blocks_ms": k, "median_fqg_bgzf_inflate_ms": med(r["fqg_bgzf_inflate_ms"]),
                      "median_device_call_ms": call, "median_host_inflate_ms": host,
                      "kernel_GBps_inflated": round(r["out_bytes"] / max(k, 1e-6) / 1e6, 2),
                      "device_call_GBps_inflated": round(r["out_bytes"] / max(call, 1e-6) / 1e6, 2),
                      "host_GBps_inflated": round(r["out_bytes"] / max(host, 1e-6) / 1e6, 2),
                      "host_over_device_call": round(host / max(call, 1e-6), 2)})
            out["files"][name] = r
    modes = {"default": {}}
    if OURS:
        modes["FQGPU_INFLATE_GPU=1"] = {"FQGPU_INFLATE_GPU": "1"}
    for name, progs in (("reads_500k", ("bam2fastq", "bam_add_tags")), ("tagged_500k", ("bam_umi_count",)),
                        ("tagged_1k", ("bam2fastq", "bam_add_tags", "bam_umi_count"))):
        path = files[name]
        for prog in progs:
            args = {"bam2fastq": ["--bam", path, "--out", os.path.join(tmp, "o")], "bam_add_tags": ["--inbam", path, "--outbam", os.path.join(tmp, "o.bam")],
                    "bam_umi_count": ["--bam", path, "--ucounts", os.path.join(tmp, "o.mtx")]}[prog]
            leg = out["programs"].setdefault(prog + " " + name, {"input_bytes": os.path.getsize(path)})
            for mode, env in modes.items():
                e = dict(os.environ)
                for k in ("FQGPU_INFLATE_GPU", "FQGPU_INFLATE_DEBUG", "FQGPU_GZIP_GPU", "FQGPU_GZIP_FAST", "FQGPU_DEVICES"):
                    e.pop(k, None)
                e.update(env)
                wall = []
                for rep in range(RUNS):
                    t0 = time.perf_counter()
                    p = subprocess.run([os.path.join(BIN, prog)] + args, env=e, capture_output=True)
                    wall.append(time.perf_counter() - t0)
                    assert p.returncode == 0, (prog, mode, p.returncode, p.stderr[-400:])
                leg[mode] = {"wall_s": [round(w, 3) for w in wall], "median_wall_s": med(wall), "spread_s": round(max(wall) - min(wall), 3)}
print(json.dumps(out, indent=1))
