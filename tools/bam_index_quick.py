"""The record index made on the device (fqg_bam_index_device, FQGPU_INDEX_GPU=1) on one box:
python tools/bam_index_quick.py [runs [bin]]

  files     the two of tools/inflate_gpu_quick.py: reads (500 000 unaligned 150-base reads) and tagged (500 000 alignments of
            tests/bamgen.py's config4), as BGZF files and as inflated streams on the device
  index     per stream: the three phases' kernel times (fqg_profile_read), the wall time of fqg_bam_index_device, and
            beside them fqg_bam_index_records - counted, then written, as the programs call it - on the same stream in the
            same process
  programs  bin/bam2fastq and bin/bam_add_tags on reads, bin/bam_umi_count on tagged: wall time, default, FQGPU_INFLATE_GPU=1,
            and FQGPU_INFLATE_GPU=1 with FQGPU_INDEX_GPU=1.  `bin`: the folder of the programs (default: this tree's), to run
            another build of them - the parent commit's, which knows the default mode only - in the same session

Every figure with its individual runs beside the median.  One JSON document on stdout.  Nothing is asserted about speed:
the numbers go to profiles/."""
import ctypes as C
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
KERNELS = ("k_bamidx_tables", "k_bamidx_follow", "k_bamidx_offsets")


def med(xs):
    return round(statistics.median(xs), 3)


out = {"runs": RUNS, "programs_of": "this tree" if OURS else "another build (the second argument)", "index": {}, "programs": {}}
with tempfile.TemporaryDirectory() as tmp:
    import torch

    import fastq_utils_amd as fq
    streams = dict(zip(("reads", "tagged"), reads_and_tagged()))
    files = {}
    for name, stream in streams.items():
        files[name] = os.path.join(tmp, name + ".bam")
        with open(files[name], "wb") as f:
            f.write(bamgen.bgzf(stream))
    if OURS:
        L = fq.abi.load()
        with fq.Context(0) as ctx:
            for name, stream in streams.items():
                rc, first, _ = fq.abi.bam_header_end(stream[:1 << 16], len(stream))
                assert rc == 0
                dev = torch.frombuffer(bytearray(stream + bytes(64)), dtype=torch.uint8).to("cuda:0")
                torch.cuda.synchronize()
                r = ctx.bam_index_device(dev.data_ptr(), len(stream), first)   # (the first call allocates)
                leg = {"stream_bytes": len(stream), "n_records": r["n_records"], "fqg_bam_index_device_ms": [], "fqg_bam_index_records_ms": []}
                leg.update({k + "_ms": [] for k in KERNELS})
                ctx.profile(True)
                for rep in range(RUNS):
                    ctx.profile_reset()
                    t0 = time.perf_counter()
                    r = ctx.bam_index_device(dev.data_ptr(), len(stream), first)
                    leg["fqg_bam_index_device_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
                    prof = ctx.profile_read()
                    for k in KERNELS:
                        leg[k + "_ms"].append(round(prof[k][1], 3))
                    leg["launches"] = {k: prof[k][0] for k in KERNELS}
                ctx.profile(False)
                n, used = C.c_uint64(), C.c_uint64()
                for rep in range(RUNS):
                    t0 = time.perf_counter()
                    L.fqg_bam_index_records(stream, len(stream), None, 0, C.byref(n), C.byref(used))
                    offs = (C.c_uint64 * max(1, n.value))()
                    L.fqg_bam_index_records(stream, len(stream), offs, n.value, C.byref(n), C.byref(used))
                    leg["fqg_bam_index_records_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
                assert (n.value, used.value) == (r["n_records"], r["used"]) and ctx.bam_index_output(n.value - 1, 1) == [offs[n.value - 1]]
                for k in list(leg):
                    if k.endswith("_ms"):
                        leg["median_" + k] = med(leg[k])
                out["index"][name] = leg
                del dev
    streams.clear()
    modes = {"default": {}}
    if OURS:
        modes["FQGPU_INFLATE_GPU=1"] = {"FQGPU_INFLATE_GPU": "1"}
        modes["FQGPU_INFLATE_GPU=1 FQGPU_INDEX_GPU=1"] = {"FQGPU_INFLATE_GPU": "1", "FQGPU_INDEX_GPU": "1"}
    for name, progs in (("reads", ("bam2fastq", "bam_add_tags")), ("tagged", ("bam_umi_count",))):
        path = files[name]
        for prog in progs:
            args = {"bam2fastq": ["--bam", path, "--out", os.path.join(tmp, "o")], "bam_add_tags": ["--inbam", path, "--outbam", os.path.join(tmp, "o.bam")],
                    "bam_umi_count": ["--bam", path, "--ucounts", os.path.join(tmp, "o.mtx")]}[prog]
            leg = out["programs"].setdefault(prog + " " + name, {"input_bytes": os.path.getsize(path)})
            for mode, env in modes.items():
                e = dict(os.environ)
                for k in ("FQGPU_INFLATE_GPU", "FQGPU_INFLATE_DEBUG", "FQGPU_INDEX_GPU", "FQGPU_INDEX_DEBUG", "FQGPU_GZIP_GPU", "FQGPU_GZIP_FAST",
                          "FQGPU_DEVICES", "FQGPU_BAMIDX_SEG", "FQGPU_BAMIDX_WINDOW", "FQGPU_BAMIDX_RING"):
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
