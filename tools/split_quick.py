"""A/B on one box, one process: fqg_records_split against the route that existed before it - two fqg_records_gather calls
with the even and the odd list - on the same frame of a device-resident synthetic interleaved image (mates 1 and 2
alternating, 150 bp).  python tools/split_quick.py [million pairs]

Prints, per route, the median over RUNS runs (after a warm-up run) of the kernel time (fqg_profile_*) and of the wall
time of the call(s), the spread of those runs, the bytes moved per record by construction and what fraction of a plain
device copy of the same bytes the kernels reach."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fastq_utils_amd as fq  # noqa: E402

RUNS = 7
pairs = int(float(sys.argv[1]) * 1e6) if len(sys.argv) > 1 else 10_000_000
n = 2 * pairs
CHUNK = 1 << 20  # records per synth call: mates alternate record by record, so the image is made in pairs of calls


def kernel_ms(prof, prefix):
    return sum(v[1] for k, v in prof.items() if k.startswith(prefix))


with fq.Context(0) as ctx:
    R = fq.abi.synth_record_bytes(150)
    # mate 1 and mate 2 images of `pairs` records each, interleaved record by record on the device
    m = [torch.empty(pairs * R, dtype=torch.uint8, device="cuda:0") for _ in (1, 2)]
    for k in (0, 1):
        ctx.synth_fastq(m[k].data_ptr(), pairs, 150, mate=k + 1)
    ctx.synchronize()
    image = torch.empty(n * R + 64, dtype=torch.uint8, device="cuda:0")
    image[: n * R].view(pairs, 2, R)[:, 0, :] = m[0].view(pairs, R)
    image[: n * R].view(pairs, 2, R)[:, 1, :] = m[1].view(pairs, R)
    torch.cuda.synchronize()
    del m
    st = fq.abi.probe_first_record(bytes(image[:4096].cpu().numpy()), True)
    r = ctx.validate(image.data_ptr(), None, st, final=True, nbytes=n * R,
                     flags=fq.abi.VALIDATE_FRAME_ONLY | fq.abi.VALIDATE_NO_STATS | fq.abi.VALIDATE_INDEX)
    assert r["n_records"] == n, r
    frame = ctx.retain_frame()
    even, odd = np.arange(0, n, 2, dtype=np.uint64), np.arange(1, n, 2, dtype=np.uint64)

    def run_split():
        return sum(ctx.records_split(frame, 0, n)[0])

    def run_gathers():
        return ctx.records_gather(frame, even)[0] + ctx.records_gather(frame, odd)[0]

    # a plain device copy of the same bytes (read n * R, write n * R)
    dst = torch.empty_like(image)
    copy_ms = []
    for _ in range(RUNS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(image)
        b.record()
        torch.cuda.synchronize()
        copy_ms.append(a.elapsed_time(b))
    del dst
    copy = statistics.median(copy_ms[1:])

    out = {"pairs": pairs, "record_bytes": R, "runs": RUNS, "device_copy_ms": round(copy, 3),
           # by construction: the record read and written once, 32 B of line index; the gathers add an 8-byte list entry
           # (uploaded and read), a 4-byte length written and read and an 8-byte offset written and read per record
           "bytes_per_record": {"split": 2 * R + 32 + 4 + 4 + 8 + 8, "two_gathers": 2 * R + 16 + 8 + 8 + 4 + 4 + 8 + 8 + 8}}
    for label, fn, prefix in (("split", run_split, "k_split"), ("two_gathers", run_gathers, "k_gather")):
        kern, wall, stats = [], [], None
        for rep in range(RUNS + 1):
            ctx.profile(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            nbytes = fn()
            ctx.synchronize()
            t1 = time.perf_counter()
            prof = ctx.profile_read()
            ctx.profile(False)
            assert nbytes == n * R, (label, nbytes)
            if rep:  # (the first run allocates the output buffers)
                kern.append(kernel_ms(prof, prefix))
                wall.append((t1 - t0) * 1e3)
                stats = {k: [v[0], round(v[1], 3)] for k, v in prof.items() if k.startswith(prefix)}
        out[label] = {"kernel_ms_median": round(statistics.median(kern), 3), "kernel_ms_min_max": [round(min(kern), 3), round(max(kern), 3)],
                      "wall_ms_median": round(statistics.median(wall), 3), "wall_ms_min_max": [round(min(wall), 3), round(max(wall), 3)],
                      "fraction_of_device_copy": round(copy / statistics.median(kern), 3), "last_run_kernels": stats}
    out["split_info"] = ctx.records_split_info()
    frame.release()
    print(json.dumps(out), flush=True)
