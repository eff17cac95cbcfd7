"""Whitelist rescue on one box: python tools/whitelist_rescue_quick.py [million reads [out.json [tree]]]

  reads      the library's synthetic reads in the BASELINE configs[2] layout (index read: 16 bp cell + 10 bp UMI, 150 bp
             cDNA), the cells drawn from a synthetic whitelist of 737 280 random 16-mers (the size of 10x's v2 list), one
             substitution planted in 0 %, 2 % and 10 % of the barcodes
  lookup     kernel time (fqg_profile_read) of k_bc_whitelist - the parent's code - and of k_bc_whitelist_correct with
             max_mismatch 0 and 1, each with and without its per-record stores (1 byte; 1 + 8 bytes); from the differences:
             what the 9 bytes per record cost, and the nanoseconds per missed barcode
  census     k_bc_census plain, with the whitelist (exact), and with the rescue, on what fqg_barcodes_transform kept
  tree       another checkout's root (the parent commit's, built): its package is measured instead, in what it has -
             k_bc_whitelist and the plain census - so that the two can take turns in one session

Medians of five runs, every run beside them.  One JSON document, written to out.json (default:
profiles/whitelist_rescue_quick.json, or ..._parent.json with a tree) and to stdout.  Nothing is asserted about speed."""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MREADS = float(sys.argv[1]) if len(sys.argv) > 1 else 8.0
TREE = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else REPO
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "whitelist_rescue_quick.json" if TREE == REPO else "whitelist_rescue_quick_parent.json")
sys.path.insert(0, TREE)
RUNS = 5
N_WL = 737_280
RATES = (0.0, 0.02, 0.10)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fastq_utils_amd as fq  # noqa: E402

A = fq.abi
assert os.path.dirname(os.path.dirname(os.path.abspath(fq.__file__))) == TREE, fq.__file__
NEW = hasattr(fq.Context, "barcodes_whitelist_correct")


def med(xs):
    return round(statistics.median(xs), 4)


def timed(ctx, kernel, call):
    """kernel milliseconds of RUNS calls (after one that is not counted)"""
    call()
    ms = []
    for _ in range(RUNS):
        ctx.profile_reset()
        call()
        prof = ctx.profile_read()
        ms.append(round(prof[kernel][1], 4))
    return {"ms": ms, "median_ms": med(ms), "spread_ms": round(max(ms) - min(ms), 4)}


n = int(MREADS * 1e6)
dev = torch.device("cuda:0")
out = {"what": __doc__.split("\n")[0], "tree": "this tree" if TREE == REPO else "another checkout (the third argument)", "reads": n,
       "whitelist_entries": N_WL, "runs": RUNS, "rates": {}}
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
    wl_codes = torch.randint(0, 4, (N_WL, 16), generator=g, device=dev)
    # char2uint_64: the first character weighs 10^0; A C G T = 1 2 3 4
    weights = np.array([10 ** p for p in range(16)], dtype=np.uint64)
    packed = ((wl_codes.cpu().numpy().astype(np.uint64) + np.uint64(1)) * weights).sum(axis=1, dtype=np.uint64)
    wl = A.Whitelist(ctx, packed.tolist())
    out["table_bytes"] = 16 * (1 << int(np.ceil(np.log2(max(1024, 4 * N_WL)))))
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
    pick = torch.randint(0, N_WL, (n,), generator=g, device=dev)
    ctx.profile(True)
    for rate in RATES:
        codes = wl_codes[pick]
        err = torch.nonzero(torch.rand(n, generator=g, device=dev) < rate).squeeze(1)
        pos = torch.randint(0, 16, (err.numel(),), generator=g, device=dev)
        codes[err, pos] = (codes[err, pos] + torch.randint(1, 4, (err.numel(),), generator=g, device=dev)) % 4   # another base
        img1.view(n, R1)[:, seq_at:seq_at + 16] = acgt[codes]
        torch.cuda.synchronize()
        del codes, pos
        r = ctx.validate(img1.data_ptr(), None, st1, final=True, flags=A.VALIDATE_FRAME_ONLY, nbytes=n * R1)
        assert r["n_records"] == n
        frame1 = ctx.retain_frame()
        leg = {"planted": int(err.numel())}
        del err
        got = ctx.barcodes_whitelist(frame1, wl, 0, 16)
        leg["n_valid"] = got["n_valid"]
        leg["k_bc_whitelist"] = timed(ctx, "k_bc_whitelist", lambda: ctx.barcodes_whitelist(frame1, wl, 0, 16))
        leg["k_bc_whitelist with its store"] = timed(ctx, "k_bc_whitelist", lambda: ctx.barcodes_whitelist(frame1, wl, 0, 16, want_flags=True))
        if NEW:
            for mm in (0, 1):
                got = ctx.barcodes_whitelist_correct(frame1, wl, 0, 16, mm)
                leg["counts max_mismatch %d" % mm] = got
                assert got["n_exact"] == leg["n_valid"]
                leg["k_bc_whitelist_correct %d" % mm] = timed(
                    ctx, "k_bc_whitelist_correct", lambda: ctx.barcodes_whitelist_correct(frame1, wl, 0, 16, mm))
                leg["k_bc_whitelist_correct %d with its stores" % mm] = timed(
                    ctx, "k_bc_whitelist_correct", lambda: ctx.barcodes_whitelist_correct(frame1, wl, 0, 16, mm, want_status=True, want_cells=True))
            base = leg["k_bc_whitelist"]["median_ms"]
            missed = n - leg["n_valid"]
            leg["derived"] = {
                "missed_barcodes": missed,
                "new kernel (0) - k_bc_whitelist, no stores, ms": round(leg["k_bc_whitelist_correct 0"]["median_ms"] - base, 4),
                "the 9 bytes per record (new kernel 1: with - without stores), ms": round(
                    leg["k_bc_whitelist_correct 1 with its stores"]["median_ms"] - leg["k_bc_whitelist_correct 1"]["median_ms"], 4),
                "the 1 byte per record (k_bc_whitelist: with - without store), ms": round(
                    leg["k_bc_whitelist with its store"]["median_ms"] - base, 4),
                "rescue (new kernel 1 - new kernel 0, no stores), ms": round(
                    leg["k_bc_whitelist_correct 1"]["median_ms"] - leg["k_bc_whitelist_correct 0"]["median_ms"], 4),
                "ns per missed barcode (new kernel 1 - k_bc_whitelist, no stores)": round(
                    (leg["k_bc_whitelist_correct 1"]["median_ms"] - base) * 1e6 / missed, 2) if missed else None,
            }
        # the census stage on what the transform keeps
        frames, states = {A.READ1: frame2, A.INDEX1: frame1}, {A.READ1: st2, A.INDEX1: st1}
        kw = dict(umi=(A.INDEX1, 16, 10), cell=(A.INDEX1, 0, 16), phred=33, min_qual=10, sam=True)
        tr = ctx.barcodes_transform(frames, states, n, **kw)
        leg["transform_kept"] = tr["n_done"] - tr["n_discarded"]

        def census(mode):
            z = ctx.census()
            if mode:
                z.set_whitelist(wl, mode - 1)
            added = ctx.barcodes_census(z, frames, states, tr["n_done"], **kw)
            info = z.whitelist_info() if mode else None
            z.close()
            return added, info

        for mode, name in ((0, "plain"), (1, "exact"), (2, "rescue")) if NEW else ((0, "plain"),):
            added, info = census(mode)
            leg["k_bc_census " + name] = dict(timed(ctx, "k_bc_census", lambda: census(mode)), pairs=added, info=info)
        frame1.release()
        out["rates"]["%g" % rate] = leg
    ctx.profile(False)
    frame2.release()
    wl.close()
text = json.dumps(out, indent=1)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(text + "\n")
print(text)
