"""The synthetic BAM streams the quick measurements share (tools/inflate_gpu_quick.py, tools/bam_index_quick.py)."""
import numpy as np


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


def reads_and_tagged(n=500000):
    """(reads, tagged): the inflated streams of n unaligned 150-base reads and of n alignments of bamgen.config4"""
    import torch

    import fastq_utils_amd as fq
    from tests import bamgen
    with fq.Context(0) as ctx:
        R = fq.abi.synth_record_bytes(150)
        img = torch.empty(n * R + 64, dtype=torch.uint8, device="cuda:0")
        ctx.synth_fastq(img.data_ptr(), n, 150)
        ctx.synchronize()
        reads = bam_of(bytes(img[:n * R].cpu().numpy()), n, R)
        del img
    rec, _, _, _ = bamgen.config4(np.random.default_rng(4), n_cells=2000, n_genes=5000, n_triples=int(n * 0.77))
    return reads, bamgen.header() + rec[:n].tobytes()
