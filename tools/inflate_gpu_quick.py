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
from tests import bamgen  # noqa: E402
from tools.quick_bam_files import reads_and_tagged  # noqa: E402

RUNS = max(3, int(sys.argv[1])) if len(sys.argv) > 1 else 5
BIN = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(REPO, "bin")
OURS = BIN == os.path.join(REPO, "bin")


def med(xs):
    return round(statistics.median(xs), 3)


out = {"runs": RUNS, "bin": os.path.relpath(BIN, REPO), "cpus_in_affinity_mask": len(os.sched_getaffinity(0)), "files": {}, "programs": {}}
with tempfile.TemporaryDirectory() as tmp:
    reads, tagged = reads_and_tagged()
    first_1k = tagged[:len(bamgen.header()) + 1000 * bamgen.REC_BYTES]
    files = {}
    for name, stream in (("reads_500k", reads), ("tagged_500k", tagged), ("tagged_1k", first_1k)):
        files[name] = os.path.join(tmp, name + ".bam")
        with open(files[name], "wb") as f:
            f.write(bamgen.bgzf(stream))
    del reads, tagged
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
