"""UMI collapse on one box: python tools/umi_collapse_quick.py [million reads [out.json]]

  reads      the library's synthetic reads in the 10x-v2 layout (index read: 16 bp cell + 10 bp UMI, 150 bp cDNA), the
             cells drawn from 5 000 random 16-mers and the UMIs of a read from 400 random 10-mers, so that a (cell, UMI)
             is read about n / 2 M times; one substitution planted in the UMI of 0 %, 2 % and 10 % of the reads
  census     transform + census of what it kept, then fqg_census_finish and fqg_census_collapse_umis (max_mismatch 1,
             and 0: the table alone) on the same pairs in the same run: kernel time (fqg_profile_read) by ProfScope
             name - k_census_finish, the yardstick, beside k_cu_flags, k_cu_rows, k_cu_run_a, k_cu_order, k_cu_run_b
             and k_cu_roots - and n_absorbed beside the number of planted errors

Medians of five runs, every run beside them.  One JSON document, written to out.json (default:
profiles/umi_collapse_quick.json) and to stdout.  Nothing is asserted about speed."""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MREADS = float(sys.argv[1]) if len(sys.argv) > 1 else 8.0
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "umi_collapse_quick.json")
sys.path.insert(0, REPO)
RUNS = 5
N_CELLS, N_UMIS = 5000, 400
RATES = (0.0, 0.02, 0.10)
KERNELS = ("k_bc_census", "k_census_finish", "k_cu_flags", "k_cu_rows", "k_cu_run_a", "k_cu_order", "k_cu_run_b", "k_cu_roots")

import torch  # noqa: E402

import fastq_utils_amd as fq  # noqa: E402

A = fq.abi


def summary(ms):
    return {"ms": ms, "median_ms": round(statistics.median(ms), 4), "spread_ms": round(max(ms) - min(ms), 4)}


n = int(MREADS * 1e6)
dev = torch.device("cuda:0")
out = {"what": __doc__.split("\n")[0], "reads": n, "cells": N_CELLS, "umis_per_cell": N_UMIS, "runs": RUNS, "rates": {}}
with fq.Context(0) as ctx:
    R1, R2 = A.synth_record_bytes(26), A.synth_record_bytes(150)
    img1 = torch.empty(n * R1, dtype=torch.uint8, device=dev)
    img2 = torch.empty(n * R2, dtype=torch.uint8, device=dev)
    ctx.synth_fastq(img1.data_ptr(), n, 26, first_index=0, seed=777, mate=1)
    ctx.synth_fastq(img2.data_ptr(), n, 150, first_index=0, seed=778, mate=2)
    ctx.synchronize()
    seq_at = bytes(img1[:R1].cpu().numpy()).index(b"\n") + 1       # the sequence line of a record
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    cell_codes = torch.randint(0, 4, (N_CELLS, 16), generator=g, device=dev)
    umi_codes = torch.randint(0, 4, (N_UMIS, 10), generator=g, device=dev)
    # barcode qualities as bench.py's barcodes extra: Phred 12..40, one base below 10 in about 5 % of the reads
    q = img1.view(n, R1)[:, seq_at + 26 + 3: seq_at + 26 + 3 + 26]
    q.clamp_(min=33 + 12)
    low = torch.nonzero(torch.rand(n, generator=g, device=dev) < 0.05).squeeze(1)
    q[low, torch.randint(0, 26, (low.numel(),), generator=g, device=dev)] = 33 + 5
    del low
    st1 = A.probe_first_record(bytes(img1[: 4 * R1].cpu().numpy()), True)
    st2 = A.probe_first_record(bytes(img2[: 4 * R2].cpu().numpy()), True)
    r = ctx.validate(img2.data_ptr(), None, st2, final=True, flags=A.VALIDATE_FRAME_ONLY, nbytes=n * R2)
    assert r["n_records"] == n
    frame2 = ctx.retain_frame()
    pick_c = torch.randint(0, N_CELLS, (n,), generator=g, device=dev)
    pick_u = torch.randint(0, N_UMIS, (n,), generator=g, device=dev)
    img1.view(n, R1)[:, seq_at:seq_at + 16] = acgt[cell_codes[pick_c]]
    ctx.profile(True)
    for rate in RATES:
        codes = umi_codes[pick_u]
        err = torch.nonzero(torch.rand(n, generator=g, device=dev) < rate).squeeze(1)
        pos = torch.randint(0, 10, (err.numel(),), generator=g, device=dev)
        codes[err, pos] = (codes[err, pos] + torch.randint(1, 4, (err.numel(),), generator=g, device=dev)) % 4   # another base
        img1.view(n, R1)[:, seq_at + 16:seq_at + 26] = acgt[codes]
        torch.cuda.synchronize()
        leg = {"planted": int(err.numel())}
        del codes, pos, err
        r = ctx.validate(img1.data_ptr(), None, st1, final=True, flags=A.VALIDATE_FRAME_ONLY, nbytes=n * R1)
        assert r["n_records"] == n
        frame1 = ctx.retain_frame()
        frames, states = {A.READ1: frame2, A.INDEX1: frame1}, {A.READ1: st2, A.INDEX1: st1}
        kw = dict(umi=(A.INDEX1, 16, 10), cell=(A.INDEX1, 0, 16), phred=33, min_qual=10, sam=True)
        tr = ctx.barcodes_transform(frames, states, n, **kw)
        leg["transform_kept"] = tr["n_done"] - tr["n_discarded"]
        for mm in (1, 0):
            runs = {k: [] for k in KERNELS}
            for i in range(RUNS + 1):   # (the first one is not counted)
                z = ctx.census()
                ctx.profile_reset()
                added = ctx.barcodes_census(z, frames, states, tr["n_done"], **kw)
                n_pairs, n_cells = z.finish()
                res = z.collapse_umis(mm)
                prof = ctx.profile_read()
                z.close()
                if i:
                    for k in KERNELS:
                        runs[k].append(round(prof[k][1], 4) if k in prof else 0.0)
            part = {k: summary(v) for k, v in runs.items()}
            total = sum(part[k]["median_ms"] for k in KERNELS if k.startswith("k_cu_"))
            part["collapse, sum of medians, ms"] = round(total, 4)
            part["collapse / k_census_finish"] = round(total / part["k_census_finish"]["median_ms"], 3)
            part.update(pairs=added, cells=n_cells, result=res)
            leg["max_mismatch %d" % mm] = part
        frame1.release()
        out["rates"]["%g" % rate] = leg
    ctx.profile(False)
    frame2.release()
text = json.dumps(out, indent=1)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(text + "\n")
print(text)
