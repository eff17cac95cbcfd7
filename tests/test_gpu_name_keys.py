"""Every way to the key of a read name, per record, at its edges.

Four pieces of device code compute the key of a header on their own - canon_name + hash_name byte by byte,
canon_name_regs + hash_name_regs on 128 bytes in registers, name_from_record from the 64-byte capture record, the
four-lane digest of the streaming pass - and a name stored through one must be found through every other.  The ladder of
tests/name_model.py puts a header at every length and blank place where they can differ (the ends of the 8-byte words, 56
/ 60 / 64 / 127 bytes, the Casava blank at either side of a word border, the longest line the reference reads whole), and
the model there says what the key is.

  - through the line index, per record: fqg_names_fingerprints_named (fingerprint, check bits, travelling name record,
    owner buckets, accounted bytes) and fqg_frame_name_records - once with the register reader wherever a line allows it,
    once in a frame that carries the NUL flag, where every header is read byte by byte;
  - capture records and digests against the line index: a name inserted one way must be found the other way.

Left out of the ladder, because no frame that holds them validates: canonical names of FQG_MAX_LABEL_LENGTH - 1 and
FQG_MAX_LABEL_LENGTH bytes (the reference reads a header line with gzgets(FQG_MAX_LABEL_LENGTH): 998 bytes and the '\\n'
are the longest line it hands out whole; the ladder has lines of 997 and 998).  The header "@" alone and a header without
'@' do not validate either (FQG_E_HDR1_SHORT / FQG_E_HDR1_AT): they are in the frames that are only framed."""
import ctypes as C
import os

import numpy as np
import pytest

import fastq_utils_amd as fq
from tests import name_model as nm

pytestmark = pytest.mark.gpu
A = fq.abi
MODE_IDS = ["%s-%s" % (s, "pe" if p else "se") for s, p in nm.MODES]
_cache = {}
NUL_HEADER = b"@~~~~\0tail"   # ('~' is in no generated name)


def ladder_headers(style, is_pe, total, lead_pads=0, degenerate=False, nul=False, mate=1, capture_order=False):
    """the header lines of an image: the lead record that fixes the format, `lead_pads` generated names, the ladder (its
    distinct names), generated names up to `total` records.  capture_order: the ladder headers that a capture record
    or a digest cannot hold come last, behind the generated names - the streaming pass does not speculate on the line
    types of an image's last chunk, so the headers that begin there are never captured, and these would not be anyway"""
    if style == "slash" and not is_pe:
        mate = 1    # (not paired: the last byte belongs to the name, so the second file holds the very same headers)
    key = (style, is_pe, total, lead_pads, degenerate, nul, mate, capture_order)
    if key not in _cache:
        fmt = nm.FMT_OF[style]
        lead = nm.lead_header(style, mate)
        ent = nm.distinct(nm.ladder(style, is_pe), fmt, is_pe, taken=[nm.canonical_name(lead, True, fmt, is_pe)])
        hs = [h for h, _ in ent]
        tail = []
        if capture_order:
            rank = lambda h: 0 if nm.holdable(h, fmt, is_pe, False) else (1 if nm.holdable(h, fmt, is_pe, True) else 2)  # noqa: E731
            tail = sorted([h for h in hs if rank(h)], key=rank)
            hs = [h for h in hs if not rank(h)]
        if mate == 2:   # the mate's header: another comment (Casava), another last byte (`slash`, paired)
            other = lambda h: (h.replace(b" 1:N:0:AC", b" 2:N:0:AC", 1) if style == "casava" else  # noqa: E731
                               (h[:-1] + b"2" if style == "slash" else h))
            hs, tail = [other(h) for h in hs], [other(h) for h in tail]
        if degenerate:
            hs += [h for h, _ in nm.degenerate(style)]
        if nul:
            hs.append(NUL_HEADER + nm.header_for(b"q", style, is_pe)[1:])
        pads = nm.generated_names(style, max(0, total - 1 - len(hs) - len(tail)) + lead_pads)
        pad_h = [nm.header_for(x, style, is_pe, mate) for x in pads]
        _cache[key] = [lead] + pad_h[:lead_pads] + hs + pad_h[lead_pads:] + tail
    return _cache[key]


def record_bytes(header, ln):
    return len(header) + 1 + 2 * (ln + 1) + 2


def unholdable_tail(headers, fmt, is_pe, digests, ln):
    """how many headers at the end of the list the format cannot hold; they must fill the image's last chunk"""
    k = 0
    while k < len(headers) and not nm.holdable(headers[len(headers) - 1 - k], fmt, is_pe, digests):
        k += 1
    assert sum(record_bytes(h, ln) for h in headers[len(headers) - k:]) >= nm.CHUNK + 4
    return k


def keys_of(headers, fmt, is_pe):
    """per record (canonical name, acct, at_sign) under the model"""
    out = []
    for h in headers:
        n, acct, at = nm.canonical(h, True, fmt, is_pe)
        out.append(((h + b"\n")[1:1 + n], acct, at))
    return out


def device_buffer(nbytes):
    import torch
    t = torch.zeros(max(1, nbytes), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()   # (torch fills it on its own stream, the library writes on the context's)
    return t


def check_line_index_keys(ctx, img, headers, style, is_pe, flags):
    L = A.load()
    fmt = nm.FMT_OF[style]
    st = A.probe_first_record(img, is_pe)
    assert st.readname_format == fmt
    r = ctx.validate(img, None, st, flags=flags)
    n = len(headers)
    assert r["n_records"] == n and r["path"] != 3, r
    if not flags & A.VALIDATE_FRAME_ONLY:
        assert r["code"] == 0, r
    keys = keys_of(headers, fmt, is_pe)
    with_at = [i for i in range(n) if keys[i][2]]
    model = {i: (nm.fingerprint(keys[i][0]), nm.check23(keys[i][0]), nm.travel_record(keys[i][0])) for i in with_at}
    base = 1000000
    for n_owners in (1, 3, 64):
        out, names = device_buffer(16 * n), device_buffer(64 * n)
        counts, nbytes = (C.c_uint64 * n_owners)(), C.c_uint64()
        ctx._check(L.fqg_names_fingerprints_named(ctx.h, None, C.byref(st), base, n_owners, C.c_void_p(out.data_ptr()),
                                                  C.c_void_p(names.data_ptr()), counts, C.byref(nbytes)))
        pairs = out.cpu().numpy().view(np.uint64).reshape(-1, 2)[:len(with_at)]
        recs = names.cpu().numpy().reshape(-1, 64)[:len(with_at)]
        want_counts = [0] * n_owners
        for i in with_at:
            want_counts[nm.owner(model[i][0], n_owners)] += 1
        assert [int(c) for c in counts] == want_counts
        assert nbytes.value == sum(keys[i][1] for i in with_at)
        seen = set()
        for k in range(len(with_at)):
            fp, word = int(pairs[k, 0]), int(pairs[k, 1])
            i = (word & nm.FP_INDEX_MASK) - base
            assert i in model and i not in seen, i
            seen.add(i)
            what = (style, is_pe, i, headers[i][:70], len(headers[i]))
            assert fp == model[i][0], what
            assert word == (base + i) | (model[i][1] << 40), what
            assert recs[k].tobytes() == model[i][2], what
            # the bucket the pair lies in is its owner's
            assert sum(want_counts[:nm.owner(fp, n_owners)]) <= k < sum(want_counts[:nm.owner(fp, n_owners) + 1]), what
        assert len(seen) == len(with_at)
    fr = ctx.retain_frame()
    assert bool(fr.h) and fr.n_records == n
    buf = device_buffer(64 * n)
    ctx.frame_name_records(fr, st, 0, n, buf.data_ptr())
    got = buf.cpu().numpy().reshape(-1, 64)
    for i in range(n):
        assert got[i].tobytes() == nm.name_record(keys[i][0], keys[i][2]), (style, is_pe, i, headers[i][:70])
    for first, cnt in ((1, 7), (n - 3, 3)):   # a range that does not start at record 0
        ctx.frame_name_records(fr, st, first, cnt, buf.data_ptr())
        got = buf.cpu().numpy().reshape(-1, 64)
        assert all(got[k].tobytes() == nm.name_record(keys[first + k][0], keys[first + k][2]) for k in range(cnt))
    fr.release()


@pytest.mark.parametrize("total", [2047, 2048, 2049])
@pytest.mark.parametrize("style,is_pe", nm.MODES, ids=MODE_IDS)
def test_line_index_keys_with_the_register_reader(style, is_pe, total):
    """one workgroup of k_names_fingerprint takes 8 x 256 records: 2047, 2048 and 2049 of them.  A validated frame; every
    header line of up to 127 bytes that does not lie in the image's last 128 bytes is read in registers."""
    headers = ladder_headers(style, is_pe, total)
    with fq.Context(0) as ctx:
        check_line_index_keys(ctx, nm.image(headers, seed=total), headers, style, is_pe, A.VALIDATE_NO_STATS)


@pytest.mark.parametrize("final_newline", [True, False], ids=["nl", "no_final_nl"])
@pytest.mark.parametrize("style,is_pe", nm.MODES, ids=MODE_IDS)
def test_line_index_keys_of_frames_that_do_not_validate(style, is_pe, final_newline):
    """the header "@" alone and a header without '@' (absent from the fingerprints, bit 63 in its name record), in a
    frame that is only framed; and a last record without its final newline, whose header lies in the last 128 bytes: the
    byte-wise reader, for a Casava header with a blank and (the record in front of it) without one"""
    headers = list(ladder_headers(style, is_pe, 300, degenerate=True))
    if style == "casava":
        headers += [b"@lastnoblank", b"@last/1 1:N:0:AC"]
    with fq.Context(0) as ctx:
        check_line_index_keys(ctx, nm.image(headers, seed=5, ln=8, final_newline=final_newline), headers, style, is_pe,
                              A.VALIDATE_FRAME_ONLY)


@pytest.mark.parametrize("style,is_pe", nm.MODES, ids=MODE_IDS)
def test_line_index_keys_with_the_byte_wise_reader(style, is_pe):
    """a header with a NUL inside validates (the reference sees a shorter C string) and raises the frame's NUL flag: every
    header of the frame is then read byte by byte - the second reader on every ladder name"""
    headers = ladder_headers(style, is_pe, 400, nul=True)
    assert any(b"\0" in h for h in headers)
    with fq.Context(0) as ctx:
        check_line_index_keys(ctx, nm.image(headers, seed=6), headers, style, is_pe, A.VALIDATE_NO_STATS)
        # the flag reached the index: the NUL header's name ends at the NUL, and a copy of that name is a repeat
        names = [k[0] for k in keys_of(headers, nm.FMT_OF[style], is_pe)]
        cut = names[[i for i, h in enumerate(headers) if b"\0" in h][0]]
        assert cut and set(cut) == {ord("~")} and names.count(cut) == 1 and len(set(names)) == len(names)
        img = nm.image(headers + [nm.header_for(cut, style, is_pe)], seed=6)
        st = A.probe_first_record(img, is_pe)
        assert ctx.validate(img, None, st, flags=A.VALIDATE_NO_STATS)["code"] == 0
        idx = ctx.name_index(4096)
        ir = idx.insert_unique(st)
        assert (ir["code"], ir["record"], ir["n_entries"]) == (nm.E_DUP_NAME, len(headers), len(headers)), ir
        idx.close()


# ---- capture records and digests against the line index --------------------------------------------------------------
READ = 60          # one read length: every chunk's speculated line type is the true one
N_CAPTURE = 700    # records: 2 * N_CAPTURE <= 4096, so an index of 8192 slots does not grow - not by a second frame either
SHIFT_PADS = 12    # generated records in front of the second arrangement: about 1.7 KiB, more than the longest header
INSERT_WAYS = {"index": (0, "0"), "pass": (A.VALIDATE_NAMES, "0"), "build": (A.VALIDATE_NAMES, "1")}


class Streamed:
    """a Context whose small images take the streaming pass (FQGPU_STREAM_MIN is read when the context is made)"""

    def __init__(self, names_build="0"):
        self.names_build = names_build

    def __enter__(self):
        os.environ["FQGPU_STREAM_MIN"] = "256"
        os.environ["FQGPU_NAMES_BUILD"] = self.names_build
        self.ctx = fq.Context(0)
        return self.ctx

    def __exit__(self, *a):
        self.ctx.close()
        os.environ.pop("FQGPU_STREAM_MIN", None)
        os.environ.pop("FQGPU_NAMES_BUILD", None)


def profiled(ctx, fn):
    ctx.profile(True)
    ctx.profile_reset()
    out = fn()
    prof = ctx.profile_read()
    ctx.profile(False)
    return out, {k for k, v in prof.items() if v[0]}


def capture_bound(headers, fmt, is_pe, digests, nbytes):
    """what names_captured() must reach: the headers the format can hold, less one per 4 KiB chunk (a chunk border can
    cost the one header that straddles it; the last chunk holds none that counts - unholdable_tail)"""
    hold = sum(1 for h in headers if nm.holdable(h, fmt, is_pe, digests))
    return hold - (nbytes + nm.CHUNK - 1) // nm.CHUNK, hold


@pytest.mark.parametrize("shift", [0, SHIFT_PADS], ids=["unshifted", "shifted"])
@pytest.mark.parametrize("way", list(INSERT_WAYS))
@pytest.mark.parametrize("style,is_pe", nm.MODES, ids=MODE_IDS)
def test_a_name_inserted_one_way_is_found_the_other_way(style, is_pe, way, shift):
    """insert through k_index_insert / k_names_pass from capture records / the LDS build from capture records; ask
    through the line index and through capture records, in reversed order (the answer comes through the hash) and in the
    same order (the positional shortcut holds the name records one way wrote against the keys the other way makes).

    A guard, not a measurement: names_captured() must reach the headers a record can hold less one per 4 KiB chunk.  Seen
    on an MI355X (captured of holdable, bound; unshifted / shifted; the same by k_names_pass and by the build): Casava
    650 of 650, 623 / 662 of 662, 634; slash paired 675 of 675, 650 / 687 of 687, 662; slash unpaired, int and nosuffix
    676 of 676, 651 / 688 of 688, 662 or 663 - every holdable header: one that runs into the next chunk is read from
    the image.  With the generated names at the end of the image, where the last chunk is never captured, the paired
    slash image fell one or two short (660 and 661 against 662): the unholdable headers were moved there."""
    fmt = nm.FMT_OF[style]
    ins_flags, build = INSERT_WAYS[way]
    h1 = ladder_headers(style, is_pe, N_CAPTURE, lead_pads=shift, capture_order=True)
    n = len(h1)
    names = [k[0] for k in keys_of(h1, fmt, is_pe)]
    assert len(set(names)) == n
    accts = [k[1] for k in keys_of(h1, fmt, is_pe)]
    model = nm.table_model(names, 8192, accts)
    img1 = nm.image(h1, seed=11, ln=READ)
    h2 = ladder_headers(style, is_pe, N_CAPTURE, lead_pads=shift, mate=2, capture_order=True)
    # reversed: the lead record stays in front (it fixes the format), the headers no record holds stay in the last chunk
    body = n - unholdable_tail(h1, fmt, is_pe, False, READ)
    order = [0] + list(range(body - 1, 0, -1)) + list(range(n - 1, body - 1, -1))
    rev, want_rev = [h2[i] for i in order], np.array(order, dtype=np.uint64)
    assert sum(1 for i in range(n) if order[i] == i) <= 3
    with Streamed(build) as ctx:
        for order, hdrs2, want in (("reversed", rev, want_rev), ("same", h2, np.arange(n, dtype=np.uint64))):
            img2 = nm.image(hdrs2, seed=12, ln=READ)
            for ask_flags in (0, A.VALIDATE_NAMES):
                st1 = A.probe_first_record(img1, is_pe)
                r = ctx.validate(img1, None, st1, flags=A.VALIDATE_NO_STATS | ins_flags)
                assert r["code"] == 0 and r["path"] == 3 and r["n_records"] == n, r
                idx = ctx.name_index(4096)
                ir, ran = profiled(ctx, lambda: idx.insert_unique(st1))
                assert (ir["code"], ir["n_entries"], ir["index_mem"]) == (0, n, model.index_mem), (ir, model.index_mem)
                cap = idx.names_captured()
                if way == "index":
                    assert cap == 0 and "k_index_insert" in ran and not ran & {"k_names_insert", "k_names_build_parts"}, ran
                else:
                    bound, hold = capture_bound(h1, fmt, is_pe, False, len(img1))
                    print("names_captured %s %s %s shift %d: %d of %d holdable, bound %d" % (style, is_pe, way, shift, cap, hold, bound))
                    assert hold > n - 60 and bound <= cap <= hold, (cap, hold, bound)
                    if way == "pass":
                        assert "k_names_insert" in ran and "k_names_build_parts" not in ran and "k_index_insert" not in ran, ran
                    else:
                        assert "k_names_build_parts" in ran and not ran & {"k_names_insert", "k_index_insert"}, ran
                st2 = A.probe_first_record(img2, is_pe)
                r = ctx.validate(img2, None, st2, flags=A.VALIDATE_NO_STATS | ask_flags)
                assert r["code"] == 0 and r["path"] == 3, r
                (mr, ans), ran = profiled(ctx, lambda: idx.probe_delete_np(st2, n))
                assert ("k_names_match" in ran) == bool(ask_flags) and ("k_index_match_delete" in ran) == (not ask_flags), ran
                bad = np.nonzero(ans != want)[0]
                assert not len(bad), (style, is_pe, way, order, ask_flags, [(int(i), hdrs2[i][:60], int(ans[i])) for i in bad[:5]])
                assert (mr["code"], mr["n_entries"]) == (0, 0), mr
                if ask_flags:
                    bound, hold = capture_bound(hdrs2, fmt, is_pe, False, len(img2))
                    assert bound <= idx.names_captured() <= hold, (idx.names_captured(), hold, bound)
                idx.close()


@pytest.mark.parametrize("shift", [0, SHIFT_PADS], ids=["unshifted", "shifted"])
@pytest.mark.parametrize("build", ["0", "1"], ids=["cas", "lds"])
@pytest.mark.parametrize("style,is_pe", nm.MODES, ids=MODE_IDS)
def test_digests_hash_a_name_as_the_line_index_does(style, is_pe, build, shift):
    """insert the image from the digests of the streaming pass, then the same image again through the line index into
    the same index: every name of the second frame must meet its first copy - a name the two ways hash differently would
    have been added.  The second call's finding is its record 0.

    names_captured() seen on an MI355X (captured of holdable, bound; unshifted / shifted; the same by CAS and by the
    build): Casava 665 of 669, 642 / 677 of 681, 653; slash 680 of 680, 655 / 692 of 692, 667; int 679 of 680, 655 /
    692 of 692, 666; nosuffix 680 of 680, 655 / 692 of 692, 667."""
    fmt = nm.FMT_OF[style]
    h1 = ladder_headers(style, is_pe, N_CAPTURE, lead_pads=shift, capture_order=True)
    n = len(h1)
    unholdable_tail(h1, fmt, is_pe, True, READ)
    keys = keys_of(h1, fmt, is_pe)
    model = nm.table_model([k[0] for k in keys], 8192, [k[1] for k in keys])
    img = nm.image(h1, seed=11, ln=READ)
    with Streamed(build) as ctx:
        st = A.probe_first_record(img, is_pe)
        r = ctx.validate(img, None, st, flags=A.VALIDATE_NO_STATS | A.VALIDATE_NAME_DIGESTS)
        assert r["code"] == 0 and r["path"] == 3, r
        idx = ctx.name_index(4096)
        idx.expect_lookups(False)
        ir, ran = profiled(ctx, lambda: idx.insert_unique(st))
        assert (ir["code"], ir["n_entries"], ir["index_mem"]) == (0, n, model.index_mem), (ir, model.index_mem)
        assert ("k_names_build_parts" in ran) == (build == "1") and ("k_names_insert" in ran) == (build == "0"), ran
        cap = idx.names_captured()
        bound, hold = capture_bound(h1, fmt, is_pe, True, len(img))
        print("names_captured (digests) %s %s build %s shift %d: %d of %d holdable, bound %d" % (style, is_pe, build, shift, cap, hold, bound))
        assert hold > n - 60 and bound <= cap <= hold, (cap, hold, bound)
        r = ctx.validate(img, None, st, flags=A.VALIDATE_NO_STATS)
        assert r["code"] == 0, r
        ir2, ran = profiled(ctx, lambda: idx.insert_unique(st))
        assert "k_index_insert" in ran and idx.names_captured() == 0
        assert (ir2["code"], ir2["record"], ir2["n_entries"], ir2["index_mem"]) == (nm.E_DUP_NAME, 0, n, model.index_mem), ir2
        idx.close()
