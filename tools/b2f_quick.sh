#!/bin/bash
# quick look at bam2fastq on the GPU: the three launches of fqg_bam2fastq (k_b2f_plan / k_b2f_scan / k_b2f_emit) on a
# seeded stream of 137-byte fastq2bam-style alignments (16 bases; on / op / CR / CY / RX / QX), GB/s of algorithmic
# bytes (the record in, the FASTQ text out).  b2f_quick.sh [alignments, default 4000000]; output under $OUT_DIR/b2f_quick
O=${OUT_DIR:-out}/b2f_quick
mkdir -p $O
python - ${1:-4000000} <<'PY' | tee $O/kernels.txt
import struct, sys
import numpy as np
import torch
import fastq_utils_amd as fq

n = int(sys.argv[1])
aux = b"onZr0000000@1:\0" + b"opZ" + b"I" * 16 + b"\0" + b"CRZACGTAC\0" + b"CYZFFFFFF\0" + b"RXZACGT\0" + b"QXZEEEE\0"
core = struct.pack("<iiIIiiii", -1, -1, (4680 << 16) | (255 << 8) | 2, (4 << 16) | 1, 16, -1, -1, 0)
body = core + b"r\0" + struct.pack("<I", 16 << 4) + bytes([0x12] * 8) + bytes([30] * 16) + aux
rec = struct.pack("<i", len(body)) + body
assert len(rec) == 137, len(rec)
hdr = b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", 0) + b"\0" * 4   # (16 bytes: the records start at a boundary)
a = np.tile(np.frombuffer(rec, dtype=np.uint8), (n, 1))
digits = np.arange(n, dtype=np.int64)
at = rec.index(b"onZr") + 4
for k in range(7):
    a[:, at + 6 - k] = 48 + digits % 10
    digits //= 10
stream = hdr + a.tobytes()
offs = (np.arange(n, dtype=np.uint64) * 137 + len(hdr))
t = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to("cuda:0")
import ctypes as C
carr = (C.c_uint64 * n).from_buffer(offs)
with fq.Context(0) as ctx:
    ctx.bam2fastq(t.data_ptr(), offsets=carr, nbytes=len(stream))   # warm-up: allocations
    ctx.profile(True)
    ctx.profile_reset()
    reps = 5
    for _ in range(reps):
        got = ctx.bam2fastq(t.data_ptr(), offsets=carr, nbytes=len(stream))
    times = ctx.profile_read()
out_bytes = sum(got["out_bytes"])
print("alignments %d, record bytes %d, FASTQ bytes per alignment %.1f" % (n, 137, out_bytes / n))
for name in ("k_b2f_plan", "k_b2f_scan", "k_b2f_emit"):
    launches, ms = times[name]
    per = ms / reps
    moved = {"k_b2f_plan": 137 * n, "k_b2f_scan": 12 * 6 * n, "k_b2f_emit": 137 * n + out_bytes}[name]
    print("%-12s %8.3f ms  %7.1f GB/s of algorithmic bytes" % (name, per, moved / per / 1e6))
PY
