// bam2fastq - drop-in for the reference program of the same name (reference src/bam2fastq.c): the reads of a BAM file
// back into FASTQ files.  A BAM written by sh/fastq2bam gives back the files it was made from (the original names and
// qualities travel in the aux tags `on` / `op`, the barcodes in CR/CY, RX/QX or UB/UY, BC/QT; -X / --10xV2 / --10xV3
// rebuild the 10x layout _R1 / _R2 / _I1), any other BAM its names, bases and qualities.  The alignment loop (:249-355)
// is one bulk call per piece of the stream into libfqgpu.so (fqg_bam2fastq, include/fqg.h).
//
// Same command line, same stderr text, same exit status; the output files inflate to the same bytes.
//   host   option parsing (getopt_long with the reference's table), BGZF inflate on all cores, the messages in the
//          order the reference prints them, gzip members on all cores
//   GPU    everything per alignment: the aux walk, the routing, base decode, quality shift, read-name repair
// There is no CPU path for the record work: without a GPU the program fails before it converts anything.
// One device (FQGPU_DEVICE); FQGPU_DEVICES is not looked at.
#include "bam_input.h"
#include <errno.h>
#include <getopt.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/fqg.h"

namespace {
using namespace fqbam;

const char kVersion[] = "0.25.3";
const char kUsage[] = "Usage: bam2fastq --bam in.bam --out fastq_prefix [--verbose --10x|-X]";
fqg_ctx* g_ctx = nullptr;

size_t piece_bytes() {  // FQGPU_CHUNK_MB: the size of the pieces in which the stream goes to the GPU
  const char* e = getenv("FQGPU_CHUNK_MB");
  size_t mb = e ? strtoull(e, nullptr, 10) : 512;
  if (mb < 1) mb = 1;
  return mb << 20;
}

// The output files: opened at the first record that writes to them (get_fp / get_10x_fp, :101-126), which is when
// the reference says so on stderr.
struct Outputs {
  const char* prefix;
  bool tenx;
  fqhost::GzipMembers gz[FQG_B2F_STREAMS];
  bool is_open[FQG_B2F_STREAMS] = {false, false, false, false, false, false};
  std::string name(int s) const {
    static const char* ext[] = {"_1", "_2", "_cell", "_sample", "_umi", ""};
    static const char* ext10[] = {"_R1", "_R2", "_I1"};
    return std::string(prefix) + (tenx ? ext10[s] : ext[s]) + ".fastq.gz";
  }
  void open(int s) {
    if (is_open[s]) return;
    const std::string n = name(s);
    if (!gz[s].open(n.c_str(), Z_DEFAULT_COMPRESSION)) {  // fastq_open(buf, "wb"), src/fastq.c:631-660
      PRINT_ERROR("Unable to open %s", n.c_str());
      leave(1);
    }
    gz[s].device(FQ_GZIP_DEVICE(g_ctx));
    is_open[s] = true;
    fprintf(stderr, "opening %s\n", n.c_str());
  }
};

}  // namespace

int main(int argc, char* argv[]) {
  char *bam_file = nullptr, *out_file_prefix = nullptr;
  static int verbose = 0, help = 0, tenx = 0;
  static struct option long_options[] = {  // :180-188
      {"verbose", no_argument, &verbose, 1}, {"help", no_argument, &help, 1}, {"bam", required_argument, 0, 'b'},
      {"out", required_argument, 0, 'o'},    {"10xV2", no_argument, &tenx, 2}, {"10xV3", no_argument, &tenx, 3},
      {0, 0, 0, 0}};
  fprintf(stderr, "bam2fastq version %s\n", kVersion);
  for (;;) {
    int option_index = 0;
    const int c = getopt_long(argc, argv, "Xb:o:h", long_options, &option_index);
    if (c == -1) break;
    switch (c) {
      case 'X': tenx = 1; break;
      case 'b': bam_file = optarg; break;
      case 'o': out_file_prefix = optarg; break;
      case 'h': help = 1; break;
      default: break;  // (unknown options are ignored, as there)
    }
  }
  if (help || bam_file == nullptr || out_file_prefix == nullptr) {  // print_usage, :165-168
    PRINT_ERROR("%s", kUsage);
    leave(help ? 0 : 1);
  }
  FILE* in = strcmp(bam_file, "-") ? fopen(bam_file, "rb") : stdin;
  if (!in) {
    fprintf(stderr, "open: %s\n", strerror(errno));  // (libbam's knetfile reports through perror("open"))
    PRINT_ERROR("Failed to open BAM file %s", bam_file);
    leave(1);
  }
  fprintf(stderr, "Processing %s\n", bam_file);

  int device = 0;
  if (const char* dev = getenv("FQGPU_DEVICE")) device = atoi(dev);
  int rc = fqg_open(device, &g_ctx);
  if (rc != 0) {
    PRINT_ERROR("no usable MI355X device (fqg_open: %d); this program has no CPU path", rc);
    leave(2);
  }
  BamInput bam;
  bam.inflate(in, bam_file, g_ctx);
  bam.index(bam_file);  // (a record cut short ends the loop, :249)
  bam.fetch_offsets();  // (the index on the device: 8 bytes per alignment come back, to cut the pieces)
  const std::vector<uint8_t>& stream = bam.stream;
  const std::vector<uint64_t>& offsets = bam.offsets;
  const uint64_t n_rec = bam.n_rec, used = bam.used;

  Outputs outs;
  outs.prefix = out_file_prefix;
  outs.tenx = tenx != 0;
  const int n_streams = tenx ? 3 : FQG_B2F_STREAMS;
  // the order in which one alignment writes to its files
  static const int rank_plain[FQG_B2F_STREAMS] = {0, 0, 1, 3, 2, 0}, rank_10x[3] = {0, 2, 1};
  bool warned = false;
  std::vector<char> text;
  const size_t piece = piece_bytes();
  uint64_t done = 0;  // alignments converted
  while (done < n_rec) {
    // a piece: whole alignments, up to `piece` bytes of the stream (one alignment at least)
    uint64_t last = done + 1;
    while (last < n_rec && last - done < 0x7FFFFFF0ull && offsets[last] + 4 - offsets[done] <= piece) ++last;
    // (a 16-byte boundary: the library stages with 16-byte loads; the offsets on the device count from byte 0 of the
    // stream, which then is what is handed over - it lies at such a boundary)
    const uint64_t p0 = bam.device_offsets ? 0 : offsets[done] & ~(uint64_t)15;
    const uint64_t p1 = last < n_rec ? offsets[last] : used;
    std::vector<uint64_t> local(bam.device_offsets ? 0 : last - done);
    for (uint64_t k = done; k < last && !bam.device_offsets; ++k) local[k - done] = offsets[k] - p0;
    fqg_b2f_params prm;
    memset(&prm, 0, sizeof(prm));
    prm.tenx = tenx != 0;
    prm.first_alignment = done;
    fqg_b2f_result res;
    rc = fqg_bam2fastq(g_ctx, bam.device ? bam.device + p0 : stream.data() + p0, p1 - p0, bam.mem(),
                       bam.device_offsets ? bam.offs(done) : local.data(), last - done, &prm, &res);
    if (rc != 0) {
      PRINT_ERROR("GPU library failure in fqg_bam2fastq (%d): %s", rc, fqg_last_error(g_ctx));
      leave(2);
    }
    // stderr as the reference's loop writes it: per alignment the progress counter (:254), the one warning (:267),
    // then an "opening" line for every file it writes to first
    struct Event {
      uint64_t record;
      int rank, what;  // what: -2 progress, -1 warning, >= 0 the stream to open
    };
    std::vector<Event> ev;
    const uint64_t seen = res.code ? res.record + 1 : res.n_alignments;  // (the alignment with the finding was counted)
    for (uint64_t k = (done / 100000 + 1) * 100000; k <= done + seen; k += 100000) ev.push_back({k - 1 - done, -2, -2});
    const bool not_fastq2bam = res.code == FQG_E_B2F_NOT_FASTQ2BAM;
    if (!warned && (res.warn_record != FQG_B2F_UNUSED || not_fastq2bam)) {
      ev.push_back({not_fastq2bam ? res.record : res.warn_record, -1, -1});
      warned = true;
    }
    for (int s = 0; s < n_streams; ++s)
      if (!outs.is_open[s] && res.first_record[s] != FQG_B2F_UNUSED) ev.push_back({res.first_record[s], tenx ? rank_10x[s] : rank_plain[s], s});
    if (res.code == FQG_E_B2F_SAMPLE_QUAL && !outs.is_open[0] && res.first_record[0] == FQG_B2F_UNUSED)
      ev.push_back({res.record, 0, 0});  // (_R1 is written before the sample's quality is missed, :314-317)
    std::sort(ev.begin(), ev.end(), [](const Event& a, const Event& b) { return a.record != b.record ? a.record < b.record : a.rank < b.rank; });
    for (const Event& e : ev) {
      if (e.what == -2) {
        fprintf(stderr, "\b\b\b\b\b\b\b\b\b\b\b\b\b\b\b%llu", (unsigned long long)(done + e.record + 1));
        fflush(stderr);
      } else if (e.what == -1) fprintf(stderr, "Warning: bam file was not generated with fastq2bam.\n");
      else outs.open(e.what);
    }
    if (res.code) {
      const unsigned long long entry = (unsigned long long)res.entry;
      switch (res.code) {
        case FQG_E_B2F_NOT_FASTQ2BAM: PRINT_ERROR("Unable to continue - bam file was not generated by fastq2bam\n"); leave(1);
        case FQG_E_B2F_CELL: PRINT_ERROR("missing cell tag in entry  %llu\n", entry); leave(3);
        case FQG_E_B2F_CELL_QUAL: PRINT_ERROR("missing cell quality tag in entry  %llu\n", entry); leave(3);
        case FQG_E_B2F_UMI: PRINT_ERROR("missing umi tag in entry  %llu\n", entry); leave(3);
        case FQG_E_B2F_UMI_QUAL: PRINT_ERROR("missing umi quality tag in entry  %llu\n", entry); leave(3);
        case FQG_E_B2F_SAMPLE_QUAL:
          PRINT_ERROR("missing sample quality tag in entry  %llu for sample %s\n", entry, bam.c_string(p0 + res.aux).c_str());
          leave(3);
        case FQG_E_B2F_TOO_LONG:
          PRINT_ERROR("%s: alignment %llu: a read of %d bases or more; the reference writes behind its %d-byte buffers there, this "
                      "program refuses the file", bam_file, entry, 10000, 10000);
          leave(2);
        default:
          PRINT_ERROR("%s: alignment %llu: an aux field, a Z value without NUL or the read name does not end inside the record; the "
                      "reference reads memory it does not own there, this program refuses the file", bam_file, entry);
          leave(2);
      }
    }
    for (int s = 0; s < n_streams; ++s) {
      if (!res.out_bytes[s]) continue;
      if (outs.gz[s].on_device()) {  // (FQGPU_GZIP_GPU=1: compressed where it lies)
        if (!outs.gz[s].write_device(FQG_TEXT_BAM2FASTQ, s)) {
          PRINT_ERROR("Failed to write %s", outs.gz[s].error().c_str());
          leave(2);
        }
        continue;
      }
      text.resize(res.out_bytes[s]);
      rc = fqg_bam2fastq_output(g_ctx, s, text.data(), res.out_bytes[s]);
      if (rc != 0) {
        PRINT_ERROR("GPU library failure in fqg_bam2fastq_output (%d): %s", rc, fqg_last_error(g_ctx));
        leave(2);
      }
      if (!outs.gz[s].write(text.data(), text.size())) {
        PRINT_ERROR("Failed to write %s", outs.gz[s].error().c_str());
        leave(2);
      }
    }
    done = last;
  }
  for (int s = 0; s < n_streams; ++s)
    if (outs.is_open[s] && !outs.gz[s].close()) {
      PRINT_ERROR("Failed to write %s", outs.gz[s].error().c_str());
      leave(2);
    }
  fprintf(stderr, "\b\b\b\b\b\b\b\b\b\b\b\b\b\b\b\n");
  fprintf(stderr, "Alignments processed: %llu\n", (unsigned long long)n_rec);
  fqg_close(g_ctx);
  leave(0);
}
