"""The device deflate compressor (fqg_deflate, FQGPU_GZIP_GPU=1) on one box: python tools/gzip_gpu_quick.py [million reads [bin]]

  kernels   GB/s of text through fqg_deflate's kernels (fqg_profile_*), the text device-resident: synthetic 150-base reads
            of fqg_synth_fastq, and the inflated FASTQ fixtures under tests/golden/data
  sizes     gzip bytes / text bytes of the same texts: the device members, zlib level 1 and the reference's level 4 on
            the same cuts, and FQGPU_GZIP_FAST's members on its own cuts (1 MiB)
  programs  wall time of bin/fastq_split_interleaved and bin/fastq_trim_poly_at on the synthetic reads (interleaved, a
            plain file) in three modes: default, FQGPU_GZIP_FAST=1, FQGPU_GZIP_GPU=1; and the size of what they wrote;
            bin/fastq_pre_barcodes with both out-files on the two mate files, in the record-block loop and in the serial
            loop (FQGPU_SERIAL_LOOP=1); bin/bam_add_tags on a BAM made from a quarter of the same reads (default and
            FQGPU_GZIP_GPU=1: FQGPU_GZIP_FAST does not apply to BGZF), with the kernel time of fqg_bgzf_deflate on its
            stream.  `bin`: the folder of the programs (default: this tree's), to run another build of them - the parent
            commit's - through the same legs in the same session

One JSON document on stdout.  No speed or size is asserted here: the numbers go to profiles/."""
import glob
import gzip
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fastq_utils_amd as fq  # noqa: E402

M = fq.abi.GZ_MEMBER_TEXT
RUNS = 5
reads = int(float(sys.argv[1]) * 1e6) if len(sys.argv) > 1 else 2_000_000
BIN = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(REPO, "bin")


def zlib_ratio(data, level, cut):
    total = 0
    for o in range(0, max(1, len(data)), cut):
        c = zlib.compressobj(level, zlib.DEFLATED, 31, 8)
        total += len(c.compress(data[o:o + cut]) + c.flush())
    return total / max(1, len(data))


def device_run(ctx, ptr, nbytes, bgzf=False):
    """(median kernel ms of the members kernel, of all deflate kernels, median wall ms, gzip bytes)"""
    kern, every, wall, size = [], [], [], 0
    for rep in range(RUNS + 1):
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        r = (ctx.bgzf_deflate if bgzf else ctx.deflate)(ptr, nbytes=nbytes, want_output=False)
        ctx.synchronize()
        t1 = time.perf_counter()
        prof = ctx.profile_read()
        ctx.profile(False)
        if rep:
            kern.append(prof["k_deflate_members"][1])
            every.append(sum(v[1] for k, v in prof.items() if k.startswith("k_deflate")))
            wall.append((t1 - t0) * 1e3)
        size = r["gz_bytes"]
    return statistics.median(kern), statistics.median(every), statistics.median(wall), size


def fast_ratio(path):
    """gzip bytes / text bytes of FQGPU_GZIP_FAST's members (1 MiB of text each) for a text file, through the check
    program of tests/cxx, which prints in=<bytes> out=<bytes>"""
    exe = os.path.join(tempfile.gettempdir(), "fastdeflate_check_%d" % os.getpid())
    if not os.path.exists(exe):
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(REPO, "tests", "cxx", "fastdeflate_check.cpp"), "-lz"], check=True)
    p = subprocess.run([exe, path, str(1 << 20)], capture_output=True, text=True, check=True)
    st = dict(kv.split("=") for kv in p.stdout.split() if "=" in kv)
    return int(st["out"]) / max(1, int(st["in"]))


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


out = {"member_text": M, "runs": RUNS, "bin": os.path.relpath(BIN, REPO), "texts": {}, "programs": {}}
with fq.Context(0) as ctx, tempfile.TemporaryDirectory() as tmp:
    R = fq.abi.synth_record_bytes(150)
    texts = {}
    img = torch.empty(reads * R + 64, dtype=torch.uint8, device="cuda:0")
    ctx.synth_fastq(img.data_ptr(), reads, 150)
    ctx.synchronize()
    texts["synth_150bp"] = bytes(img[:reads * R].cpu().numpy())
    fixtures = b"".join(gzip.open(p).read() for p in sorted(glob.glob(os.path.join(REPO, "tests", "golden", "data", "c18_10000_*.fastq.gz"))))
    texts["fixtures_c18_10000"] = fixtures
    for name, data in texts.items():
        dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        k_ms, all_ms, wall_ms, size = device_run(ctx, dev.data_ptr(), len(data))
        sample = data[:64 * M]  # (zlib on one core: a sample of 4 MB says what the ratio is)
        path = os.path.join(tmp, name + ".txt")
        with open(path, "wb") as f:
            f.write(sample)
        out["texts"][name] = {
            "bytes": len(data), "members": -(-len(data) // M),
            "k_deflate_members_ms": round(k_ms, 3), "deflate_kernels_ms": round(all_ms, 3), "call_wall_ms": round(wall_ms, 3),
            "kernel_GBps": round(len(data) / all_ms / 1e6, 2), "call_GBps": round(len(data) / wall_ms / 1e6, 2),
            "ratio_device": round(size / len(data), 4),
            "ratio_device_sample": round(ctx.deflate(sample, want_output=False)["gz_bytes"] / len(sample), 4),
            "ratio_zlib_1_sample": round(zlib_ratio(sample, 1, M), 4), "ratio_zlib_4_sample": round(zlib_ratio(sample, 4, M), 4),
            "ratio_zlib_4_1MiB_members_sample": round(zlib_ratio(sample, 4, 1 << 20), 4),
            "ratio_gzip_fast_sample": round(fast_ratio(path), 4),
        }
        del dev
    del img
modes = {"default": {}, "FQGPU_GZIP_FAST=1": {"FQGPU_GZIP_FAST": "1"}, "FQGPU_GZIP_GPU=1": {"FQGPU_GZIP_GPU": "1"}}
# the programs on synthetic reads, mates alternating (an interleaved file); the context that made them is closed before
# the programs start: they open the device themselves
with tempfile.TemporaryDirectory() as tmp:
    src = os.path.join(tmp, "reads.fastq")
    with fq.Context(0) as ctx:
        half = (reads // 2) * 2
        R = fq.abi.synth_record_bytes(150)
        m = [torch.empty((half // 2) * R, dtype=torch.uint8, device="cuda:0") for _ in (1, 2)]
        for k in (0, 1):
            ctx.synth_fastq(m[k].data_ptr(), half // 2, 150, mate=k + 1)
        ctx.synchronize()
        inter = torch.empty(half * R, dtype=torch.uint8, device="cuda:0")
        inter.view(half // 2, 2, R)[:, 0, :] = m[0].view(half // 2, R)
        inter.view(half // 2, 2, R)[:, 1, :] = m[1].view(half // 2, R)
        torch.cuda.synchronize()
        with open(src, "wb") as f:
            f.write(bytes(inter.cpu().numpy()))
        del m, inter
        # the mates as two files, and an unaligned BAM of a quarter of the reads (the stream compressed by the device: any
        # BGZF file does as input)
        mates = [os.path.join(tmp, "r%d.fastq" % k) for k in (1, 2)]
        with open(src, "rb") as f:
            both = np.frombuffer(f.read(), dtype=np.uint8).reshape(half // 2, 2, R)
        for k in (0, 1):
            with open(mates[k], "wb") as f:
                f.write(both[:, k, :].tobytes())
        n_bam = half // 4
        stream = bam_of(both.tobytes(), n_bam, R)
        del both
        bam = os.path.join(tmp, "reads.bam")
        with open(bam, "wb") as f:
            f.write(ctx.bgzf_deflate(stream)["members"])
        dev = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        k_ms, all_ms, wall_ms, size = device_run(ctx, dev.data_ptr(), len(stream), bgzf=True)
        out["texts"]["bam_stream_bgzf"] = {"bytes": len(stream), "blocks": -(-len(stream) // M), "k_deflate_members_ms": round(k_ms, 3),
                                           "deflate_kernels_ms": round(all_ms, 3), "call_wall_ms": round(wall_ms, 3),
                                           "kernel_GBps": round(len(stream) / all_ms / 1e6, 2), "ratio_device": round(size / len(stream), 4)}
        bam_bytes = len(stream)
        del dev, stream
    text_bytes = os.path.getsize(src)
    barcodes = ["--read1", mates[0], "--read2", mates[1], "--umi_read", "read1", "--umi_offset", "0", "--umi_size", "8", "--read1_offset", "8",
                "--phred_encoding", "33", "--outfile1", os.path.join(tmp, "o1.fastq.gz"), "--outfile2", os.path.join(tmp, "o2.fastq.gz")]
    serial = {"FQGPU_SERIAL_LOOP": "1"}
    host_only = {m: v for m, v in modes.items() if "FAST" not in m}
    for leg, prog, args, extra, leg_modes, in_bytes in (
            ("fastq_split_interleaved", "fastq_split_interleaved", [src, os.path.join(tmp, "o")], {}, modes, text_bytes),
            ("fastq_trim_poly_at", "fastq_trim_poly_at", ["--file", src, "--outfile", os.path.join(tmp, "o.fastq.gz")], {}, modes, text_bytes),
            ("fastq_pre_barcodes (block loop)", "fastq_pre_barcodes", barcodes, {}, modes, text_bytes),
            ("fastq_pre_barcodes (serial loop)", "fastq_pre_barcodes", barcodes, serial, modes, text_bytes),
            ("bam_add_tags", "bam_add_tags", ["--inbam", bam, "--outbam", os.path.join(tmp, "o.bam.gz")], {}, host_only, bam_bytes)):
        out["programs"][leg] = {"input_bytes": in_bytes}
        for mode, env in leg_modes.items():
            e = dict(os.environ)
            for k in ("FQGPU_GZIP_GPU", "FQGPU_GZIP_FAST", "FQGPU_GZIP_LEVEL", "FQGPU_SERIAL_LOOP", "FQGPU_DEVICES"):
                e.pop(k, None)
            e.update(extra)
            e.update(env)
            wall = []
            for rep in range(3):
                t0 = time.perf_counter()
                p = subprocess.run([os.path.join(BIN, prog)] + args, env=e, capture_output=True)
                wall.append(time.perf_counter() - t0)
                assert p.returncode == 0, p.stderr[-400:]
            written = sum(os.path.getsize(p) for p in glob.glob(os.path.join(tmp, "o*.gz")))
            text = sum(len(gzip.open(p).read()) for p in glob.glob(os.path.join(tmp, "o*.gz")))
            out["programs"][leg][mode] = {"wall_s": [round(w, 3) for w in wall], "median_wall_s": round(statistics.median(wall), 3),
                                          "gz_bytes": written, "ratio": round(written / in_bytes, 4), "text_bytes": text,
                                          "ratio_of_text": round(written / max(1, text), 4)}
            for p in glob.glob(os.path.join(tmp, "o*.gz")):
                os.remove(p)
print(json.dumps(out, indent=1))
