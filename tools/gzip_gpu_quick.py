"""The device deflate compressor (fqg_deflate, FQGPU_GZIP_GPU=1) on one box: python tools/gzip_gpu_quick.py [million reads]

  kernels   GB/s of text through fqg_deflate's kernels (fqg_profile_*), the text device-resident: synthetic 150-base reads
            of fqg_synth_fastq, and the inflated FASTQ fixtures under tests/golden/data
  sizes     gzip bytes / text bytes of the same texts: the device members, zlib level 1 and the reference's level 4 on
            the same cuts, and FQGPU_GZIP_FAST's members on its own cuts (1 MiB)
  programs  wall time of bin/fastq_split_interleaved and bin/fastq_trim_poly_at on the synthetic reads (interleaved, a
            plain file) in three modes: default, FQGPU_GZIP_FAST=1, FQGPU_GZIP_GPU=1; and the size of what they wrote

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
import torch  # noqa: E402

import fastq_utils_amd as fq  # noqa: E402

M = fq.abi.GZ_MEMBER_TEXT
RUNS = 5
reads = int(float(sys.argv[1]) * 1e6) if len(sys.argv) > 1 else 2_000_000


def zlib_ratio(data, level, cut):
    total = 0
    for o in range(0, max(1, len(data)), cut):
        c = zlib.compressobj(level, zlib.DEFLATED, 31, 8)
        total += len(c.compress(data[o:o + cut]) + c.flush())
    return total / max(1, len(data))


def device_run(ctx, ptr, nbytes):
    """(median kernel ms of the members kernel, of all deflate kernels, median wall ms, gzip bytes)"""
    kern, every, wall, size = [], [], [], 0
    for rep in range(RUNS + 1):
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        r = ctx.deflate(ptr, nbytes=nbytes, want_output=False)
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


out = {"member_text": M, "runs": RUNS, "texts": {}, "programs": {}}
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
    text_bytes = os.path.getsize(src)
    for prog, args in (("fastq_split_interleaved", [src, os.path.join(tmp, "o")]),
                       ("fastq_trim_poly_at", ["--file", src, "--outfile", os.path.join(tmp, "o.fastq.gz")])):
        out["programs"][prog] = {"input_bytes": text_bytes}
        for mode, env in modes.items():
            e = dict(os.environ)
            for k in ("FQGPU_GZIP_GPU", "FQGPU_GZIP_FAST", "FQGPU_GZIP_LEVEL"):
                e.pop(k, None)
            e.update(env)
            wall = []
            for rep in range(3):
                t0 = time.perf_counter()
                p = subprocess.run([os.path.join(REPO, "bin", prog)] + args, env=e, capture_output=True)
                wall.append(time.perf_counter() - t0)
                assert p.returncode == 0, p.stderr[-400:]
            written = sum(os.path.getsize(p) for p in glob.glob(os.path.join(tmp, "o*.gz")))
            out["programs"][prog][mode] = {"wall_s": [round(w, 3) for w in wall], "median_wall_s": round(statistics.median(wall), 3),
                                           "gz_bytes": written, "ratio": round(written / text_bytes, 4)}
            for p in glob.glob(os.path.join(tmp, "o*.gz")):
                os.remove(p)
print(json.dumps(out, indent=1))
