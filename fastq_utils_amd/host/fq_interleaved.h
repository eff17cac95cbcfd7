// fq_interleaved.h - which finding the reference's interleaved loop hits first (src/fastq_info.c:72-101 and the same
// loop in src/fastq_split_interleaved.c:59-89), decided from the bulk results of one image: its validation
// (fqg_validate) and the comparison of the names of its pairs (fqg_names_compare on the frame alone).  Shared by
// fastq_info ("pe": the whole file is one image) and fastq_split_interleaved (piece by piece: pair and line numbers go
// on from piece to piece, and only the piece that ends the file can be truncated).  Included behind fq_common.h.
#pragma once
#include "fq_common.h"

namespace {

struct InterleavedImage {
  const char* path;
  const char* data;  // the image: it starts at a record boundary
  size_t size;
  uint64_t n;         // records of the image that count: all it framed when it ends the file, an even number otherwise
  bool ends_file;     // an incomplete last record / a first mate without a second are findings
  uint64_t pair_base; // pairs in front of this image
};

// Order inside pair k: read m1, read m2, name m1, name m2, names equal, validate m1, validate m2.  Prints the format
// lines where the first fastq_get_readname prints them (probe_pending: no pair has got that far yet) and leaves with
// the image's first finding; returns when it has none.
void interleaved_findings(const InterleavedImage& im, const fqg_validate_result& r, const fqg_index_result& cr, const Probe& pr,
                          bool& probe_pending) {
  const uint64_t n = im.n;
  uint64_t best_pair = ~0ull;
  int best_stage = 99;
  auto offer = [&](uint64_t pair, int stage) {
    if (pair < best_pair || (pair == best_pair && stage < best_stage)) {
      best_pair = pair;
      best_stage = stage;
    }
  };
  // (a record behind the even prefix of an image that does not end the file is looked at again with the next image)
  const bool counts = r.code && (im.ends_file || r.record < n);
  const bool trunc = counts && (r.code == FQG_E_TRUNCATED || r.code == FQG_E_LINE_TOO_LONG);
  if (trunc) offer(r.record / 2, r.record % 2 == 0 ? 0 : 2);
  else if (counts && r.code == FQG_E_HDR1_AT) offer(r.record / 2, r.record % 2 == 0 ? 3 : 4);
  else if (counts) offer(r.record / 2, r.record % 2 == 0 ? 6 : 7);
  if (im.ends_file) {
    if (r.tail_lines > 0) offer(n / 2, n % 2 == 0 ? 0 : 2);  // an incomplete last record, even when an earlier record has a finding
    else if (n % 2 == 1) offer(n / 2, 1);                     // a first mate without a second one
  }
  if (cr.code == FQG_E_WRONG_HEADER) {
    const RecordText t = locate_record(im.data, im.size, cr.record);
    offer(cr.record / 2, (!t.l[0].empty() && t.l[0][0] != '@') ? 3 : 4);
  }
  if (cr.code == FQG_E_UNPAIRED) offer(cr.record / 2, 5);
  // format lines: printed by the first fastq_get_readname call, i.e. for mate 1 of pair 0
  if (probe_pending && n >= 2) {
    if (!(best_pair == 0 && best_stage <= 3)) print_probe(pr);
    probe_pending = false;
  }
  if (best_pair == ~0ull) return;
  ticker(im.pair_base + 1, im.pair_base + best_pair, 50000, 2);
  const uint64_t k = best_pair, rec_base = 2 * im.pair_base;
  const unsigned long cline_pair = 4 * (rec_base + 2 * k + 2);
  switch (best_stage) {
    case 0:
    case 2:
      if (r.code == FQG_E_LINE_TOO_LONG) fail_too_long(im.path, rec_base + r.record);
      fail_truncated(im.path, 4 * (rec_base + best_pair * 2 + (best_stage == 2 ? 1 : 0)));
    case 1:
      FQ_PRINT_ERROR("Error in file %s: line %lu: file truncated?", im.path, (unsigned long)(4 * (rec_base + n)));
      fqhost::leave(kExitFormat);
    case 3:
      fail_wrong_header(im.path, cline_pair, locate_record(im.data, im.size, 2 * k).l[0]);
    case 4:
      fail_wrong_header(im.path, cline_pair, locate_record(im.data, im.size, 2 * k + 1).l[0]);
    case 5:
      FQ_PRINT_ERROR("Error in file %s: line %lu: unpaired read - %s", im.path, cline_pair,
                     canonical_name(locate_record(im.data, im.size, 2 * k).l[0], pr.st).c_str());
      fqhost::leave(kExitFormat);
    default:
      print_validation_error(im.path, cline_pair, r, locate_record(im.data, im.size, r.record));
      fqhost::leave(kExitFormat);
  }
}

}  // namespace
