// fastq_split_interleaved - drop-in for the reference program of the same name (reference
// src/fastq_split_interleaved.c): one interleaved FASTQ file into <prefix>_1.fastq.gz and <prefix>_2.fastq.gz.
//
// Same command line, stdout, stderr and exit status; the two outputs hold the same records in the same order (what a
// reader inflates is identical).  What runs where:
//   GPU    framing + validation of a piece (fqg_validate), the names of its pairs (fqg_names_compare on the frame
//          alone), the de-interleave of its records into two texts (fqg_records_split)
//   host   reading / inflating the input, deflating the outputs on every core (fq_parallel.h, the reference's level 4),
//          which finding comes first and its wording (fq_interleaved.h, shared with fastq_info's "pe" mode)
// The file goes through PIECE BY PIECE: a piece that frames an odd number of records hands its last record, with the
// unfinished tail behind it, to the next piece; pair numbers, line numbers and the progress counter go on across pieces.
// One device (FQGPU_DEVICE; of FQGPU_DEVICES the first ordinal).
#include <unistd.h>

#include <string>
#include <vector>

#include "fq_common.h"
#include "fq_interleaved.h"
#include "fq_multi.h"
#include "fq_parallel.h"

namespace {

using Out = fqhost::GzipMembers;

// fastq_new(path, FALSE, "w4") -> fastq_open (src/fastq.c:631-664)
Out* open_out(const std::string& path) {
  Out* g = new Out();
  if (!g->open(path.c_str(), 4)) {
    FQ_PRINT_ERROR("Unable to open %s", path.c_str());
    fqhost::leave(kExitParams);
  }
  g->device(FQ_GZIP_DEVICE(g_ctx));
  return g;
}

void written(Out* out, bool ok) {
  if (!ok) {
    FQ_PRINT_ERROR("%s.\n", out->error().c_str());  // GZ_WRITE's gzerror() text, src/fastq.c:211-235
    fqhost::leave(kExitSys);
  }
}

void close_out(Out* g) {  // fastq_destroy -> fastq_close (src/fastq.c:615-629)
  if (!g->close()) {
    FQ_PRINT_ERROR("unable to close file descriptor");
    fqhost::leave(kExitSys);
  }
  delete g;
}

}  // namespace

int main(int argc, char** argv) {
  fqhost::install_counted_output(argv);  // (fq_respawn.h: a run that starts over on input cut at the gzgets limits prints nothing twice)
  fprintf(stderr, "fastq_utils %s\n", "0.25.3");  // fastq_print_version
  if (argc != 3) {
    FQ_PRINT_ERROR("Usage: fastq_split_interleaved interleaved_fastq out_prefix");
    fqhost::leave(kExitParams);
  }
  const char* path = argv[1];
  const std::string prefix = argv[2];
  // (the reference builds the two names in char[1024] with sprintf: "_1.fastq.gz" is eleven characters and the NUL)
  if (prefix.size() >= 1012) {
    FQ_PRINT_ERROR("out_prefix of %zu characters: the reference's file name buffers hold 1011", prefix.size());
    fqhost::leave(kExitSys);
  }
  const std::vector<int> devices = devices_from_env();
  const char* dev = getenv("FQGPU_DEVICE");
  const int ordinal = !devices.empty() ? devices[0] : dev ? atoi(dev) : 0;
  if (!devices.empty()) fprintf(fqhost::diag(), "fqgpu: fastq_split_interleaved runs on one device: taking %d, the first of FQGPU_DEVICES\n", ordinal);
  fqhost::keep_slots_until_exit() = true;
  const int rc = fqg_open(ordinal, &g_ctx);
  if (rc != 0) {
    FQ_PRINT_ERROR("no usable MI355X device (fqg_open: %d); this program has no CPU path", rc);
    fqhost::leave(kExitSys);
  }
  fprintf(stderr, "Paired-end interleaved\n");
  Input in(g_ctx, path, piece_bytes());  // ("Unable to open ...": before any output file exists)
  Out* w[2] = {open_out(prefix + "_1.fastq.gz"), open_out(prefix + "_2.fastq.gz")};
  fqg_acc* acc = nullptr;
  LIB(fqg_acc_create(g_ctx, &acc));

  Probe pr;
  uint64_t pair_base = 0;
  bool probe_pending = true;
  std::vector<char> host[2];
  while (in.next()) {
    probe_piece(pr, in.data(), in.size(), 1);
    fqg_validate_result r;
    LIB(fqg_validate(g_ctx, acc, in.data(), in.size(), FQG_MEM_HOST, in.final() ? 1 : 0, &pr.st, FQG_VALIDATE_INDEX | in.vflags(), &r));
    // (a NUL byte at a record start ends the file there, src/fastq.c:250)
    const bool ends_file = in.final() || r.stopped;
    // a piece that framed an odd number of records: the last one waits for its mate in the next piece
    const bool odd = !ends_file && (r.n_records & 1);
    uint64_t carry_at = r.consumed;
    if (odd) {
      fqg_record last;
      LIB(fqg_frame_records(g_ctx, r.n_records - 1, 1, &last, FQG_MEM_HOST));
      carry_at = last.offset;
    }
    const uint64_t n = odd ? r.n_records - 1 : r.n_records;
    fqg_frame* fr = nullptr;
    fqg_index_result cr{};
    if (r.n_records >= 2) {
      LIB(fqg_frame_retain(g_ctx, &fr));
      LIB(fqg_names_compare(g_ctx, fr, &pr.st, nullptr, nullptr, &cr));
    }
    interleaved_findings(InterleavedImage{path, in.data(), in.size(), n, ends_file, pair_base}, r, cr, pr, probe_pending);
    // no finding: n is even, and every pair of the piece is written
    if (n) {
      uint64_t bytes[2] = {0, 0};
      LIB(fqg_records_split(g_ctx, fr, 0, n, bytes));
      if (w[0]->on_device()) {  // (FQGPU_GZIP_GPU=1: both texts are compressed where they lie)
        for (int s = 0; s < 2; ++s) written(w[s], w[s]->write_device(FQG_TEXT_RECORDS, 1 + s));
      } else {
        for (int s = 0; s < 2; ++s) {
          if (host[s].size() < bytes[s]) host[s].resize(bytes[s]);
          LIB(fqg_records_split_output(g_ctx, s, host[s].data(), bytes[s]));
        }
        for (int s = 0; s < 2; ++s) written(w[s], w[s]->write(host[s].data(), bytes[s]));
      }
    }
    if (fr) fqg_frame_release(fr);
    ticker(pair_base + 1, pair_base + n / 2, 50000, 2);  // PRINT_READS_PROCESSED(cline / 4, 100000) behind every pair
    pair_base += n / 2;
    if (ends_file) break;
    in.carry_from(carry_at);
  }
  printf("\n");
  close_out(w[0]);
  close_out(w[1]);
  fqhost::leave(0);
}
