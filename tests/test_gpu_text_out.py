"""The contract of the output text that stays on the device (fqg_text_out.inc) as the six producers' `_output` calls
show it: fqg_barcodes_transform, fqg_records_filter, fqg_records_gather, fqg_records_split, fqg_bam_add_tags and
fqg_bam2fastq.  What was produced can be copied in full or as a prefix and no byte more; a call without records leaves
nothing to copy; the text of a BAM call survives a FASTQ-side call; a copy that is still on its way is waited for by
the next producer; fqg_release_scratch gives the FASTQ side's text back.  2048 + 3 records per stream: every scan has a
second span, so the span sums are in play."""
import ctypes as C

import numpy as np
import pytest

import fastq_utils_amd as fq
from oracle import bam_tags_oracle as bto
from oracle import filter_oracle as fo
from oracle import pre_barcodes_oracle as pbo
from tests import b2f_gen, bamgen, split_gen
from tests import bam2fastq_oracle as b2f

pytestmark = pytest.mark.gpu
A = fq.abi
N = 2048 + 3
ERR_ARG = -3  # FQG_ERR_ARG, include/fqg.h


def ten_x(seed, n):
    """(barcode reads: 16 bp cell + 10 bp UMI, cDNA reads of about 50 bp), the same names before the blank"""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    r1, r2 = [], []
    for i in range(n):
        name = b"@TXT:1:FC:%d:%d:%d" % (i % 8 + 1, i % 97, i)
        q1 = (rng.integers(12, 41, 26) + 33).astype(np.uint8)
        if rng.random() < 0.05:
            q1[int(rng.integers(0, 26))] = 33 + 5  # below --min_qual: the pair is discarded
        l2 = int(rng.integers(45, 56))
        r1.append(name + b" 1:N:0:ACGT\n" + bases[rng.integers(0, 4, 26)].tobytes() + b"\n+\n" + q1.tobytes() + b"\n")
        r2.append(name + b" 2:N:0:ACGT\n" + bases[rng.integers(0, 4, l2)].tobytes() + b"\n+\n" +
                  (rng.integers(2, 41, l2) + 33).astype(np.uint8).tobytes() + b"\n")
    return b"".join(r1), b"".join(r2)


def tagged_stream(seed, n):
    """(a BAM stream of n short alignments whose names carry barcodes, its reference names)"""
    rng = np.random.default_rng(seed)
    names = [b"TX%04d.%d" % (i, i % 3) for i in range(12)]
    recs = []
    for i in range(n):
        name = b"STAGS_CELL=%s_UMI=%s_SAMPLE=%s_ETAGS_M%d" % (bamgen.barcode(rng, 16), bamgen.barcode(rng, 10),
                                                             bamgen.barcode(rng, int(rng.choice([0, 8]))), i)
        recs.append(bamgen.record(name, b"", tid=int(rng.integers(-1, 12)), seq_len=int(rng.integers(45, 56))))
    return bamgen.header(tuple((nm, 1000) for nm in names)) + b"".join(recs), names


def fastq2bam_stream(seed, n):
    """a BAM stream of n alignments as fastq2bam writes them: every one of the six streams gets text"""
    rng = np.random.default_rng(seed)
    return b2f_gen.stream([b2f_gen.fastq2bam_record(rng, i, paired=i % 3 != 0, sample=True, long_read=45 + i % 11) for i in range(n)])


class Producer:
    """One producing call on inputs of its own.  run(): {stream id: the text the oracle gives}; run_empty(): the same
    call without records; output(): the call's `_output` as the C-ABI has it -> (status, bytes)."""

    def __init__(self, ctx, seed):
        self.ctx, self.seed, self.frames = ctx, seed, []

    def frame_of(self, image):
        st = A.probe_first_record(image[:4096], True)
        r = self.ctx.validate(image, None, st, final=True, flags=A.VALIDATE_FRAME_ONLY | A.VALIDATE_NO_STATS | A.VALIDATE_INDEX)
        assert r["code"] == 0
        self.frames.append(self.ctx.retain_frame())
        return self.frames[-1], st

    def copy(self, fn, *args):
        nbytes = args[-1]
        buf = C.create_string_buffer(max(1, nbytes))
        rc = fn(self.ctx.h, *args[:-1], buf, nbytes)
        return rc, buf.raw[:nbytes]

    def close(self):
        for f in self.frames:
            f.release()


class Transform(Producer):
    def __init__(self, ctx, seed):
        super().__init__(ctx, seed)
        r1, r2 = ten_x(seed, N)
        (f2, st2), (f1, st1) = self.frame_of(r2), self.frame_of(r1)
        self.args = ({A.READ1: f2, A.INDEX1: f1}, {A.READ1: st2, A.INDEX1: st1})
        self.kw = dict(umi=(A.INDEX1, 16, 10), cell=(A.INDEX1, 0, 16), phred=33, min_qual=10, sam=True)
        files = {"i1.fastq": r1, "r1.fastq": r2}
        want = pbo.run_pre_barcodes(["--read1", "r1.fastq", "--index1", "i1.fastq", "--umi_read", "index1", "--umi_offset", "16",
                                     "--umi_size", "10", "--cell_read", "index1", "--cell_offset", "0", "--cell_size", "16",
                                     "--phred_encoding", "33", "--min_qual", "10", "--sam", "--outfile1", "-"], files.get)
        assert want["exit"] == 0
        self.want = {0: "".join(ln + "\n" for ln in want["stdout"].splitlines() if not ln.startswith("@")).encode("latin-1")}

    def run(self, n=N):
        r = self.ctx.barcodes_transform(*self.args, n, **self.kw)
        assert r["code"] == 0 and r["n_done"] == n and r["out_bytes"][0] == (len(self.want[0]) if n else 0)
        return self.want

    def run_empty(self):
        self.run(0)

    def output(self, s, nbytes):
        return self.copy(A.load().fqg_barcodes_output, s, nbytes)


class Filter(Producer):
    def __init__(self, ctx, seed):
        super().__init__(ctx, seed)
        image = b"".join(split_gen.pairs(seed, (N + 1) // 2, len1=(45, 56))[:N])
        self.frame, _ = self.frame_of(image)
        self.want = {0: fo.filter_n(["in.fastq"], lambda p: image)["stdout"]}

    def run(self, n=N):
        r = self.ctx.records_filter(self.frame, n, A.FILTER_N, max_n_percent=0)
        assert r["n_records"] == n and r["out_bytes"] == (len(self.want[0]) if n else 0)
        return self.want

    def run_empty(self):
        self.run(0)

    def output(self, s, nbytes):
        return self.copy(A.load().fqg_records_filter_output, nbytes)


class Gather(Producer):
    def __init__(self, ctx, seed):
        super().__init__(ctx, seed)
        recs = split_gen.pairs(seed, (N + 1) // 2, style="slash", len1=(45, 56))[:N]
        self.frame, _ = self.frame_of(b"".join(recs))
        self.order = np.random.default_rng(seed).permutation(N).astype(np.uint64)
        self.want = {0: b"".join(recs[int(k)] for k in self.order)}

    def run(self):
        nbytes, _ = self.ctx.records_gather(self.frame, self.order)
        assert nbytes == len(self.want[0])
        return self.want

    def run_empty(self):
        assert self.ctx.records_gather(self.frame, self.order[:0])[0] == 0

    def output(self, s, nbytes):
        return self.copy(A.load().fqg_records_gather_output, nbytes)


class Split(Producer):
    def __init__(self, ctx, seed):
        super().__init__(ctx, seed)
        image = b"".join(split_gen.pairs(seed, N, len1=(45, 56), len2=(40, 61)))
        self.frame, _ = self.frame_of(image)
        self.want = dict(enumerate(split_gen.deinterleave(image)))

    def run(self):
        sizes, _ = self.ctx.records_split(self.frame, 0, 2 * N)
        assert sizes == (len(self.want[0]), len(self.want[1]))
        return self.want

    def run_empty(self):
        assert self.ctx.records_split(self.frame, 0, 0)[0] == (0, 0)

    def output(self, s, nbytes):
        return self.copy(A.load().fqg_records_split_output, s, nbytes)


class BamTags(Producer):
    def __init__(self, ctx, seed):
        super().__init__(ctx, seed)
        self.stream, self.names = tagged_stream(seed, N)
        out, n = bto.add_tags_stream(self.stream, tx_tag=True)
        self.first = bto.parse_header(self.stream)[1]
        assert n == N
        self.want = {0: out[self.first:]}

    def run(self):
        r = self.ctx.bam_add_tags(self.stream, tx_tag=True, targets=self.names, want_output=False)
        assert r["code"] == 0 and r["n_alignments"] == N and r["out_bytes"] == len(self.want[0])
        return self.want

    def run_empty(self):
        r = self.ctx.bam_add_tags(self.stream[:self.first], tx_tag=True, targets=self.names, want_output=False)
        assert r["code"] == 0 and r["n_alignments"] == 0 and r["out_bytes"] == 0

    def output(self, s, nbytes):
        return self.copy(A.load().fqg_bam_add_tags_output, nbytes)


class Bam2Fastq(Producer):
    def __init__(self, ctx, seed):
        super().__init__(ctx, seed)
        self.stream = fastq2bam_stream(seed, N)
        want = b2f.convert(self.stream)
        assert want["fatal"] is None and want["n_alignments"] == N and all(want["streams"])
        self.want = {s: bytes(t) for s, t in enumerate(want["streams"])}

    def run(self):
        r = self.ctx.bam2fastq(self.stream)
        assert r["code"] == 0 and r["out_bytes"] == [len(self.want[s]) for s in range(6)]
        return self.want

    def run_empty(self):
        r = self.ctx.bam2fastq(self.stream[:bto.parse_header(self.stream)[1]])
        assert r["code"] == 0 and r["n_alignments"] == 0 and r["out_bytes"] == [0] * 6

    def output(self, s, nbytes):
        return self.copy(A.load().fqg_bam2fastq_output, s, nbytes)


KINDS = {"transform": Transform, "filter": Filter, "gather": Gather, "split": Split, "bam_add_tags": BamTags, "bam2fastq": Bam2Fastq}


@pytest.fixture(scope="module")
def ctx():
    with fq.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def producer(ctx):
    """producer(kind, seed=0): made once (inputs, frames, the oracle's text), shared by the tests"""
    made = {}

    def get(kind, seed=0):
        if (kind, seed) not in made:
            made[(kind, seed)] = KINDS[kind](ctx, 100 * seed + list(KINDS).index(kind))
        return made[(kind, seed)]

    yield get
    for p in made.values():
        p.close()


def holds(p, want):
    """every stream of the last call of p can be copied in full, and is the oracle's text"""
    for s, text in want.items():
        assert p.output(s, len(text)) == (0, text), s


def nothing_to_copy(p, want):
    for s in want:
        assert p.output(s, 0) == (0, b"")
        assert p.output(s, 1)[0] == ERR_ARG


@pytest.mark.parametrize("kind", list(KINDS))
def test_bounds_and_prefix(producer, kind):
    p = producer(kind)
    want = p.run()
    holds(p, want)
    for s, text in want.items():
        assert len(text) > 4096
        for nbytes in (1, 4097, len(text) - 1):
            assert p.output(s, nbytes) == (0, text[:nbytes]), (s, nbytes)
        assert p.output(s, 0) == (0, b"")
        assert p.output(s, len(text) + 1)[0] == ERR_ARG
        assert "more than" in A.load().fqg_last_error(p.ctx.h).decode()
    holds(p, want)  # (a refused copy changes nothing)


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_call_without_records_leaves_nothing_to_copy(producer, kind):
    p = producer(kind)
    want = p.run()
    holds(p, want)
    p.run_empty()
    nothing_to_copy(p, want)


@pytest.mark.parametrize("bam, fastq", [("bam_add_tags", "filter"), ("bam2fastq", "split")])
def test_bam_and_fastq_sides_do_not_disturb_each_other(producer, bam, fastq):
    b, f = producer(bam), producer(fastq)
    want_b = b.run()
    want_f = f.run()
    holds(b, want_b)
    holds(f, want_f)
    want_b = b.run()  # ... and the other way round
    holds(f, want_f)
    holds(b, want_b)


@pytest.mark.parametrize("second", ["split", "gather"])
def test_a_copy_on_its_way_is_awaited_by_the_next_producer(ctx, producer, second):
    L = A.load()
    first, nxt = producer("split", seed=1), producer(second)
    text = first.run()[1]
    host = L.fqg_host_alloc(ctx.h, len(text))
    assert host
    try:
        C.memset(host, 0, len(text))
        assert L.fqg_barcodes_output_begin(ctx.h, 2, C.c_void_p(host), len(text)) == 0  # (the split's stream 1)
        want = nxt.run()
        assert L.fqg_barcodes_output_wait(ctx.h) == 0
        assert C.string_at(host, len(text)) == text
        assert all(t != text[:len(t)] for t in want.values())
        holds(nxt, want)
    finally:
        L.fqg_host_free(ctx.h, C.c_void_p(host))


@pytest.mark.parametrize("kind", ["transform", "filter", "gather", "split"])
def test_release_scratch_gives_the_text_back(ctx, producer, kind):
    p = producer(kind)
    want = p.run()
    holds(p, want)
    ctx.release_scratch()
    nothing_to_copy(p, want)
    holds(p, p.run())  # (and the next call allocates again)
