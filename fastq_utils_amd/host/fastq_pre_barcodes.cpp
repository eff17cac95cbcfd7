// fastq_pre_barcodes - drop-in for the reference program of the same name
// (reference src/fastq_pre_barcodes.c): same options, same stderr / stdout text, same output bytes.
//
//   host   option parsing, (gz) reading of up to five inputs into pinned pieces, lock-step
//          bookkeeping across pieces, gzip / stdout writing of what the GPU produced
//   GPU    framing of every input, read-name agreement, barcode extraction with the quality
//          filter, header tagging, slicing, and the assembly of the output text (FASTQ or SAM)
// --bam (not an option of the reference): what `fastq_pre_barcodes --sam ... | samtools view -b -` writes in the
// reference's sh/fastq2bam, without the pipe - the GPU makes the alignment records samtools 0.1.19 makes of the SAM
// lines, the program writes the BGZF file to stdout.
// There is no CPU path for the per-read work.
#include <getopt.h>
#include <unistd.h>

#include <chrono>
#include <deque>
#include <functional>
#include <set>
#include <string>
#include <vector>

#include "fq_blocks.h"
#include "fq_common.h"
#include "fq_multi.h"
#include "fq_ordered.h"
#include "fq_out_pool.h"
#include "fq_parallel.h"

// SURVEY 5 "metrics", as bin/fastq_info has it: FQGPU_JSON_METRICS=<file> writes the machine-readable twin of the
// "Reads processed / discarded" lines - the command line and both output streams stay the reference's
static const std::chrono::steady_clock::time_point g_pb_start = std::chrono::steady_clock::now();
static void pb_json_metrics(long processed, long discarded, size_t devices) {
  const char* jm = getenv("FQGPU_JSON_METRICS");
  if (!jm) return;
  FILE* jf = fopen(jm, "w");
  if (!jf) return;
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - g_pb_start).count();
  const unsigned long long bytes = fqhost::bytes_handed_out().load();
  fprintf(jf, "{\"program\": \"fastq_pre_barcodes\", \"reads\": %ld, \"discarded\": %ld, \"input_bytes\": %llu, \"seconds\": %.6f, "
              "\"Mreads_per_s\": %.3f, \"GB_per_s\": %.3f, \"devices\": %zu}\n",
          processed, discarded, bytes, secs, secs > 0 ? (double)processed / secs / 1e6 : 0.0, secs > 0 ? (double)bytes / secs / 1e9 : 0.0,
          devices ? devices : (size_t)1);
  fclose(jf);
}

namespace {

enum { READ1 = 1, READ2 = 2, INDEX1 = 3, INDEX2 = 4, INDEX3 = 5 };

int read_index2read_idx(const char* s) {  // src/fastq_pre_barcodes.c:79-89
  if (!strcmp(s, "read1")) return READ1;
  if (!strcmp(s, "read2")) return READ2;
  if (!strcmp(s, "index1")) return INDEX1;
  if (!strcmp(s, "index2")) return INDEX2;
  if (!strcmp(s, "index3")) return INDEX3;
  FQ_PRINT_ERROR("invalid file reference %s (valid values are read1,read2, index1,index2,index3)\n", s);
  fqhost::leave(1);
}

void print_usage() {  // src/fastq_pre_barcodes.c:311-346
  const char msg[] =
      "  --verbose    :increase level of messages printed to stderr\n"
      "  --brief      :decrease level of messages printed to stderr\n"
      "  --help       :print the usage\n"
      "  --read1 <filename> :fastq (optional gzipped) file name \n"
      "  --read2 <filename> :fastq (optional gzipped) file name \n"
      "  --index1 <filename> :fastq (optional gzipped) file name \n"
      "  --index2 <filename> :fastq (optional gzipped) file name \n"
      "  --index3 <filename> :fastq (optional gzipped) file name \n"
      "  --phred_encoding (33|64) :phred encoding used in the input files\n"
      "  --min_qual [0-40]        :defines the minimum quality that all bases in the UMI, CELL or Sample should "
      "have (reads that do not pass the criteria are discarded). 0 disables the filter. \n"
      "  --outfile1 <filename>    :file name for ouputing the reads from file1\n"
      "  --outfile2 <filename>    :file name for ouputing the reads from file2\n"
      "  --outfile3 <filename>    :file name for ouputing the reads from file3\n"
      "  --interleaved (read1|read2|index1|index2|index3),(read1|read2|index1|index2|index3)    :interleaved data\n"
      "  --umi_read (read1|read2|index1|index2|index3)       :in which input file can the UMI be found\n"
      "  --umi_offset integer     :offset \n"
      "  --umi_size               :number of bases after the offset\n"
      "  --cell_read (read1|read2|index1|index2|index3)      :in which input file can the cell be found\n"
      "  --cell_offset integer    :offset \n"
      "  --cell_size integer      :number of bases after the offset\n"
      "  --sample_read (read1|read2|index1|index2|index3)    :in which input file can the sample barcode be found\n"
      "  --sample_offset integer  :offset \n"
      "  --sample_size integer    :number of bases after the offset\n"
      "  --read1_offset integer   :\n"
      "  --read1_size integer     :\n"
      "  --read2_offset integer   :\n"
      "  --read2_size integer     :\n"
      "  --10x     : use 10X UMI tags (UB and UY) instead of the default tags defined in the SAM specification\n";
  // (--bam is not listed: the usage text is the reference's, byte for byte; README.md and DESIGN.md 4.5 describe it)
  fprintf(stderr, "usage: fastq_pre_barcodes --read1 fastq_file --outfile1 out_file [optional parameters]\n");
  fprintf(stderr, "%s\n", msg);
}

// The reference reads a line beyond its gzgets buffers in pieces (src/fastq.c:249-253) and goes on out of step, every
// piece a line of its own.  Everything in front of this piece of input went the reference's way; the program runs itself
// again, as a child and on one device, on input that is cut where gzgets cuts it (fq_respawn.h, fq_reframe.h: inflated
// input is cut while it is read and never comes here) - every piece a line, a C string to the kernels as to the
// reference.  Only a stream that cannot be read twice is refused.
std::function<void()> g_before_respawn;  // (the one-device loop: text still on its way to stdout is written first)
[[noreturn]] void refuse_long_line(const char* path, uint64_t record) {
  if (fqhost::reframe_supported() && !fqhost::reframing() && strcmp(path, "-") != 0) {
    if (g_before_respawn) g_before_respawn();
    fqhost::respawn_reframed();
  }
  FQ_PRINT_ERROR("Error in file %s: record %lu has a line longer than the reference's line buffers (%d / %d bytes)", path,
                 (unsigned long)(record + 1), FQG_MAX_LABEL_LENGTH - 1, FQG_MAX_READ_LENGTH - 1);
  fflush(stdout);
  fqhost::leave(kExitSys);
}

// ---- what the two loops share: how a piece of input is framed, what a batch says and counts once
// fqg_barcodes_transform has returned, how its text comes back and is written, and how the run ends -----------------

// A piece of one input that starts at a record boundary, framed.  A header line that starts with a NUL byte is "no
// entry" for the reference (src/fastq.c:250): the input ends HERE, cleanly, whatever follows, and the records in front of
// it are framed once more, alone.  Another line of a record that starts with NUL is an empty string: the file is
// truncated THERE (src/fastq.c:254; tail_lines > 0), whatever follows.
struct Framed {
  fqg_validate_result r{};
  bool ends_here = false, cut_short = false;
  bool final = false;     // no record of the input lies behind this piece
  int tail_lines = 0;
  bool open_end = false;  // the file's last line has no '\n' and closes its last complete record: gzgets reads it up
                          // to the end of the file, and the file is at its end for gzeof from then on
};
// 0, or the status of the library call *what that failed.  A line beyond the gzgets limits comes back as
// f->r.code == FQG_E_LINE_TOO_LONG with nothing else decided; the frame is the caller's to retain.
int frame_piece(fqg_ctx* c, const char* data, size_t size, bool final, const fqg_file_state* st, uint32_t flags, Framed* f,
                const char** what) {
  *f = Framed{};
  *what = "fqg_validate";
  fqg_validate_result& r = f->r;
  int rc = fqg_validate(c, nullptr, data, size, FQG_MEM_HOST, final ? 1 : 0, st, FQG_VALIDATE_FRAME_ONLY | flags, &r);
  if (rc || r.code == FQG_E_LINE_TOO_LONG) return rc;
  f->ends_here = r.stopped != 0;
  if (f->ends_here && (rc = fqg_validate(c, nullptr, data, r.consumed, FQG_MEM_HOST, 1, st, FQG_VALIDATE_FRAME_ONLY | flags, &r))) return rc;
  f->cut_short = !f->ends_here && r.code == FQG_E_TRUNCATED && !final;
  f->final = final || f->ends_here || f->cut_short;
  f->tail_lines = f->ends_here ? 0 : r.tail_lines;
  f->open_end = final && !f->ends_here && r.tail_lines == 0 && r.n_records > 0 && size > 0 && data[size - 1] != '\n';
  return 0;
}

// how an input stood when its loop ended
struct InputEnd {
  bool drained = false;     // nothing of it is left for another iteration, and nothing more will come
  bool at_end = false;      // the next read would begin exactly behind its last complete record ...
  bool one_beyond = false;  // ... or one record further (the serial loop's second --interleaved reference)
  bool open_end = false;    // Framed::open_end of its last piece
  int tail_lines = 0;       // lines of an incomplete record behind the last complete one
  uint64_t records = 0;     // complete records of the file up to there
};

// the header line of a FQG_E_WRONG_HEADER finding, and its line number by the file's own counter (src/fastq.c:448-451)
struct WrongHeader {
  unsigned long line;
  std::string text;
};

// --bam: the BGZF file on stdout.  Host mode: the records come back as they are and the host's threads compress them
// (zlib's default level, as bam_add_tags does).  Device mode (FQGPU_GZIP_GPU=1, loops on one context): every batch's
// records are compressed where they lie (fqg_text_bgzf_deflate) with the carry chain of the gzip files - the header is
// the first carry -, and what is left when the loop ends becomes the last block.  Either way the blocks are cut at
// multiples of 65280 bytes of the stream and the end-of-file block closes the file.
struct BamOut {
  bool on = false, device = false;
  fqhost::BgzfStream host;
  std::string* carry = nullptr;  // device mode: the loop's carry of output 0
  bool close(fqg_ctx* c) {
    if (!device) return host.close();
    fqg_deflate_result dr;
    if (fqg_bgzf_deflate(c, carry->data(), carry->size(), nullptr, 0, FQG_MEM_HOST, 1, &dr)) return false;
    std::vector<char> last(dr.gz_bytes);
    if (fqg_deflate_output(c, last.data(), last.size())) return false;
    return fwrite(last.data(), 1, last.size(), stdout) == last.size();
  }
};
BamOut g_bam;
std::string g_bam_header;  // device mode: the first carry of output 0

struct Batches {
  const char* const* file = nullptr;
  const fqg_barcode_params* P = nullptr;
  GzipMembers* outgz = nullptr;
  int num_input_files = 0;
  uint64_t scale = 1;  // 2 with --interleaved input: an iteration takes two reads of the file, the ticker counts reads
  Probe pr[6];         // state of every input's first record + the line fastq_get_readname prints on its first call
  unsigned long processed = 0, discarded = 0;
  bool first = true;

  // Before the batch's text goes out: the format lines of the first fastq_get_readname call per file, in file order
  // (src/fastq.c:459-485) - up to the file whose first header is wrong -, and the warnings.
  void announce(const fqg_barcode_result& r) {
    if (first && num_input_files > 1)
      for (int x = READ1; x <= INDEX3; ++x)
        if (file[x]) {
          if (r.code == FQG_E_WRONG_HEADER && r.iteration == 0 && r.file == x) break;
          print_probe(pr[x]);
        }
    first = false;
    for (uint64_t w = 0; w < r.n_short; ++w) fputs("Warning: Read too short - barcode not found\n", stderr);
  }
  // Behind it: the counters, the ticker and - after `flush` has brought out what the loop still holds - the finding
  // that ends the run.
  void count(const fqg_barcode_result& r, const std::function<void()>& flush, const std::function<WrongHeader()>& wrong_header) {
    const unsigned long before = processed;
    processed += r.n_done;
    discarded += r.n_discarded;
    ticker(before + 1, processed, 100000, scale);
    if (r.code == FQG_OK) return;
    flush();
    if (r.code == FQG_E_WRONG_HEADER) {
      const WrongHeader h = wrong_header();
      fail_wrong_header(file[r.file], h.line, h.text);
    }
    if (r.code == FQG_E_BAM_RECORD) {  // (not a reference outcome: samtools view -b would abort on this line, or worse)
      FQ_PRINT_ERROR("read #%ld: the SAM line of read%d cannot be written as a BAM record (empty or mismatched sequence / quality, "
                     "an empty tag value, or a tab, a line break or a byte >= 0x80 where libbam cannot take one)", (long)(processed + 1), r.file);
      fqhost::leave(2);
    }
    FQ_PRINT_ERROR("Readnames do not match across files (read #%ld)", (long)(processed + 1));
    fqhost::leave(kExitFormat);
  }
  // The loop is over.  An incomplete record where the next read would have happened is a truncated file
  // (src/fastq.c:254-257); a clean end of any input just ends the loop.  The first input, in file order, that has nothing
  // left decides - unless the loop's own condition ends it first (fastq_files_eof, src/fastq_pre_barcodes.c:288-297,
  // :594): an input whose last line has no '\n' is at its end for gzeof once that line has been read, and no input is
  // read again.
  [[noreturn]] void finish(const InputEnd* end, size_t devices) {
    bool loop_condition_ends_it = false;
    for (int x = READ1; x <= INDEX3; ++x)
      if (file[x] && end[x].drained && end[x].at_end && end[x].open_end) loop_condition_ends_it = true;
    for (int x = READ1; x <= INDEX3 && !loop_condition_ends_it; ++x)
      if (file[x] && end[x].drained) {
        if (end[x].tail_lines > 0 && (end[x].at_end || end[x].one_beyond)) fail_truncated(file[x], (unsigned long)(4 * end[x].records));
        break;
      }
    FQ_PRINT_INFO("Reads processed: %ld", (long)processed);
    FQ_PRINT_INFO("Reads discarded: %ld", (long)discarded);
    if (!P->out_sam)
      for (int x = READ1; x <= READ2; ++x)
        if (P->emit[x] && !outgz[x].close()) {
          FQ_PRINT_ERROR("unable to close file descriptor");
          fqhost::leave(kExitSys);
        }
    if (g_bam.on && !g_bam.close(g_ctx)) {
      FQ_PRINT_ERROR("unable to write the BAM file to stdout");
      fqhost::leave(kExitSys);
    }
    fflush(stdout);
    pb_json_metrics((long)processed, (long)discarded, devices);
    fqhost::leave(0);
  }
};

// One output's text of one batch on its way from the GPU to its file: `size` bytes in a buffer of the pool - the
// text, or (FQGPU_GZIP_GPU=1, loops on one context) gz_bytes of gzip members and behind them the text that filled none.
struct OutText {
  char* buf = nullptr;
  size_t cap = 0, size = 0, gz_bytes = 0;
  bool members = false;
};

// The fetch step for output `which` of the transform that has just run on `c`: in device mode the text is compressed
// where it lies, `carry` (the tail of the batch before, docs/host_gzip.md section 3) in front; a buffer of the pool;
// the copy into it - `beside`: on the library's copy stream, beside what the caller does next, until fetch_wait; else
// made when this returns (fqg_*_output is a copy on the context's own stream, not _begin + _wait).
// 0, or the status of the call *what that failed.
int fetch_begin(fqg_ctx* c, OutPool& pool, int which, size_t text_bytes, bool device_mode, const std::string& carry, bool beside,
                OutText* o, const char** what) {
  *o = OutText{};
  o->members = device_mode;
  o->size = text_bytes;
  if (o->members) {
    fqg_deflate_result dr;
    *what = which == 0 ? "fqg_text_bgzf_deflate" : "fqg_text_deflate";
    if (const int rc = which == 0 ? fqg_text_bgzf_deflate(c, FQG_TEXT_RECORDS, 0, carry.data(), carry.size(), 0, &dr)  // (--bam)
                                  : fqg_text_deflate(c, FQG_TEXT_RECORDS, which, carry.data(), carry.size(), 0, &dr))
      return rc;
    o->gz_bytes = dr.gz_bytes;
    o->size = dr.gz_bytes + dr.tail_bytes;
  }
  *what = "no pinned memory for the output text";
  if (!(o->buf = pool.take(o->size, &o->cap))) return FQG_ERR_NOMEM;
  if (o->members) {
    *what = beside ? "fqg_deflate_output_begin" : "fqg_deflate_output";
    return beside ? fqg_deflate_output_begin(c, o->buf, o->size) : fqg_deflate_output(c, o->buf, o->size);
  }
  *what = beside ? "fqg_barcodes_output_begin" : "fqg_barcodes_output";
  return beside ? fqg_barcodes_output_begin(c, which, o->buf, o->size) : fqg_barcodes_output(c, which, o->buf, o->size);
}
// ... and its end: the copy has landed, and the tail that came with it is the carry of the next batch
int fetch_wait(fqg_ctx* c, const OutText& o, std::string* carry) {
  const int rc = o.members ? fqg_deflate_output_wait(c) : fqg_barcodes_output_wait(c);
  if (!rc && o.members) carry->assign(o.buf + o.gz_bytes, o.size - o.gz_bytes);
  return rc;
}
// the write step (0: the SAM text to stdout, or --bam: the records through the host compressor / the blocks the device
// made of them; device mode: the members, and the tail for close())
bool write_out(GzipMembers* gz, int which, const OutText& o) {
  if (which == 0 && g_bam.on) return o.members ? fwrite(o.buf, 1, o.gz_bytes, stdout) == o.gz_bytes : g_bam.host.write(o.buf, o.size);
  if (which == 0) return fwrite(o.buf, 1, o.size, stdout) == o.size;
  return o.members ? gz[which].write_members(o.buf, o.gz_bytes, o.buf + o.gz_bytes, o.size - o.gz_bytes) : gz[which].write(o.buf, o.size);
}
size_t outputs_per_batch(const fqg_barcode_params& P) {
  return P.out_sam ? 1 : std::max<size_t>((size_t)((P.emit[1] ? 1 : 0) + (P.emit[2] ? 1 : 0)), 1);
}

// ---- the serial loop's input: pieces, frames, and where the next iteration reads ------------------------------------
struct Source {
  Input* in = nullptr;
  Probe* pr = nullptr;  // (Batches::pr)
  fqg_frame* frame = nullptr;
  uint64_t avail = 0;           // complete records in the current frame
  long use = 0;                 // local index of the record the next iteration uses (may exceed avail)
  uint64_t records_before = 0;  // records in earlier frames
  Framed f;                     // the current piece
  bool exhausted = false;       // no more data will come
  bool carry_pending = false;
  size_t carry_at = 0;          // bytes of the current piece covered by complete records
};

// frame the next piece of `s`; false when the input is used up
bool refill(Source& s) {
  if (s.frame) {
    fqg_frame_release(s.frame);
    s.frame = nullptr;
    s.records_before += s.avail;
    s.use -= (long)s.avail;
    s.avail = 0;
  }
  if (s.exhausted) return false;
  if (s.carry_pending) {  // only now: the piece's bytes stay readable for messages until it is replaced
    s.in->carry_from(s.carry_at);
    s.carry_pending = false;
  }
  if (!s.in->next()) {
    s.exhausted = true;
    return false;
  }
  probe_piece(*s.pr, s.in->data(), s.in->size(), 1);
  const char* what;
  if (const int rc = frame_piece(g_ctx, s.in->data(), s.in->size(), s.in->final(), &s.pr->st, s.in->vflags(), &s.f, &what)) die_lib(what, rc);
  if (s.f.r.code == FQG_E_LINE_TOO_LONG) refuse_long_line(s.in->path().c_str(), s.records_before + s.f.r.record);
  s.avail = s.f.r.n_records;
  if (s.avail) LIB(fqg_frame_retain(g_ctx, &s.frame));
  if (!s.f.final) {
    s.carry_pending = true;
    s.carry_at = s.f.r.consumed;
  } else s.exhausted = true;
  return s.avail > 0 || !s.exhausted;
}

// What a batch of the serial loop prints goes to a writer thread (in order: one thread, one queue): gzip'ing and writing
// batch k - the reference's whole cost in FASTQ mode - runs beside reading, framing and transforming batch k + 1.  Two
// batches may wait; drain() before anything else may be said or the program leaves.
struct OutJob {
  int which = 0;
  OutText t;
};
struct AsyncOut {
  GzipMembers* gz;
  OutPool* pool;  // (where a buffer goes once it is written)
  std::deque<OutJob> q;
  std::mutex mu;
  std::condition_variable cv;
  bool quit = false, failed = false, busy = false;
  std::thread th;
  double t_write = 0;
  void start() {
    th = std::thread([this] {
      for (;;) {
        OutJob j;
        {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return quit || !q.empty(); });
          if (q.empty()) return;
          j = std::move(q.front());
          q.pop_front();
          busy = true;
        }
        const auto t0 = std::chrono::steady_clock::now();
        const bool ok = write_out(gz, j.which, j.t);
        pool->give(j.t.buf, j.t.cap);
        {
          std::lock_guard<std::mutex> lk(mu);
          t_write += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
          if (!ok) failed = true;
          busy = false;
        }
        cv.notify_all();
      }
    });
  }
  void push(const OutJob& j) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return q.size() < 2; });
    q.push_back(j);
    lk.unlock();
    cv.notify_all();
  }
  bool drain() {  // everything handed over is written; false: a write failed
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return q.empty() && !busy; });
    return !failed;
  }
  void stop() {
    {
      std::lock_guard<std::mutex> lk(mu);
      quit = true;
    }
    cv.notify_all();
    if (th.joinable()) th.join();
  }
};

// ---- the loop over record blocks: every input is cut into blocks of the same B records (fq_blocks.h), block j of all
// inputs is one unit, whichever context is free takes the next unit (FQGPU_DEVICES=0,1,..: several GPUs), and the main
// thread takes the results in unit order - what the serial loop prints and writes, in its order.  Not for --interleaved
// input (a discarded read leaves the reference's file pointers out of step from there on,
// src/fastq_pre_barcodes.c:653 vs :722: a serial dependence).
struct Unit {
  uint64_t seq = 0;
  int rc = 0;
  std::string err;
  fqg_barcode_result r{};
  uint64_t n = 0;                 // iterations the unit had to offer
  Framed f[6];                    // every input's block
  bool ends = false;              // an input ends inside this unit although its block is not the last
  int long_line_file = 0;         // an input of this unit has a line beyond the gzgets limits ...
  uint64_t long_line_record = 0;  // ... in this record of the file
  OutText out[3];                 // the text of every output
  std::string wrong_header;       // the text of the header line of a FQG_E_WRONG_HEADER finding
  Block b[6];                     // the context's thread's: given back before the unit is handed over
};

struct BlockLoop {
  Batches& A;
  const std::vector<fqg_ctx*> ctx;  // (ctx[0]: g_ctx)
  RecordBlocks* cut[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  uint64_t B = 1;
  // units under way or waiting for the writer: one per context and one more; none is begun beyond that (a context that
  // ran ahead would hold every buffer with units the writer cannot take yet, and the unit it waits for would find none)
  const uint64_t window;
  OutPool out_pool;  // as many buffers as the units that may be under way have outputs
  // The carry chain of the device compressor, one per output file: the context's thread's alone.  With ONE context every
  // unit passes through that thread in unit order (fq_ordered.h), so the tail of unit k is the carry of unit k + 1; the
  // thread that writes never calls into the context while units are under way.
  std::string gz_carry[3] = {g_bam_header, std::string(), std::string()};
  const bool timing = getenv("FQGPU_TIMING") != nullptr;
  struct UnitTimes {  // FQGPU_TIMING: one context's seconds
    double frame = 0, transform = 0, out = 0;
  };
  std::vector<UnitTimes> T;
  static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

  BlockLoop(Batches& a, const std::vector<int>& devs)
      : A(a), ctx(fqhost::open_more_contexts(g_ctx, devs)), window(devs.size() + 1),
        out_pool(FQ_PINNED_ALLOC(g_ctx), (size_t)window * outputs_per_batch(*a.P)), T(devs.size()) {
    g_bam.carry = &gz_carry[0];
    double record_bytes = 64;
    for (int x = READ1; x <= INDEX3; ++x)
      if (A.file[x]) {
        cut[x] = new RecordBlocks(g_ctx, A.file[x], (int)devs.size() + 2);
        probe_piece(A.pr[x], cut[x]->peek(), cut[x]->peek_size(), 1);
        const double rb = cut[x]->peek_lines() >= 4 ? 4.0 * (double)cut[x]->peek_size() / (double)cut[x]->peek_lines()
                                                    : (double)std::max<size_t>(cut[x]->peek_size(), 64);
        record_bytes = std::max(record_bytes, rb);
      }
    B = std::max<uint64_t>(1, (uint64_t)((double)piece_bytes(128) / record_bytes));
    if (const char* e = getenv("FQGPU_BLOCK_RECORDS")) B = std::max<uint64_t>(1, strtoull(e, nullptr, 10));  // (tests: tiny blocks)
    for (int x = READ1; x <= INDEX3; ++x)
      if (cut[x]) cut[x]->start(B);
  }

  // block `seq` of every input (false only after an abort: a unit that holds the end of an input is the last one handed out)
  bool next_unit(uint64_t seq, Unit& u, bool& last) {
    for (int x = READ1; x <= INDEX3; ++x)
      if (cut[x] && !cut[x]->next(&u.b[x])) return false;
    u.seq = seq;
    for (int x = READ1; x <= INDEX3; ++x)
      if (cut[x] && u.b[x].final) last = true;
    return true;
  }
  static void lib_fail(fqg_ctx* c, Unit& u, const char* what, int rc) {
    u.rc = rc;
    u.err = std::string(what) + ": " + fqg_last_error(c);
  }
  // frame the unit's blocks; held[x]: the retained frame of input x
  void frame_unit(fqg_ctx* c, Unit& u, const fqg_file_state* states, fqg_frame** held) {
    u.n = ~0ull;
    for (int x = READ1; x <= INDEX3; ++x)
      if (cut[x]) {
        const Block& b = u.b[x];
        Framed& f = u.f[x];
        const char* what;
        if (const int rc = frame_piece(c, b.data, b.size, b.final, &states[x], 0, &f, &what)) return lib_fail(c, u, what, rc);
        if (f.r.code == FQG_E_LINE_TOO_LONG) {  // (the thread that takes the results starts the program over: refuse_long_line)
          u.long_line_file = x;
          u.long_line_record = u.seq * B + f.r.record;
          u.rc = FQG_ERR_ARG;
          return;
        }
        if (f.ends_here || f.cut_short) u.ends = true;  // the last unit the consumer looks at
        if (!f.final && (f.r.n_records != B || f.r.consumed != b.size)) {
          u.rc = FQG_ERR_STATE;
          u.err = std::string("a block of ") + A.file[x] + " cut at a record boundary was not consumed whole";
          return;
        }
        u.n = std::min<uint64_t>(u.n, f.r.n_records);
        if (f.r.n_records)
          if (const int rc = fqg_frame_retain(c, &held[x])) return lib_fail(c, u, "fqg_frame_retain", rc);
      }
  }
  // transform the unit and fetch its text (and the header text of a wrong-header finding: the blocks are given back)
  void transform_unit(size_t di, fqg_ctx* c, Unit& u, const fqg_file_state* states, fqg_frame* const* held) {
    const double t2 = timing ? now() : 0;
    const uint64_t first[6] = {0, 0, 0, 0, 0, 0};
    fqg_barcode_params Pb = *A.P;
    if (const int rc = fqg_barcodes_transform(c, held, states, first, &Pb, u.n, u.seq * B, &u.r)) lib_fail(c, u, "fqg_barcodes_transform", rc);
    const double t3 = timing ? now() : 0;
    T[di].transform += t3 - t2;
    for (int which = 0; which < 3 && !u.rc; ++which)
      if (u.r.out_bytes[which]) {
        const char* what;
        // (a device was handed over to the output files for one context only: main)
        if (const int rc = fetch_begin(c, out_pool, which, u.r.out_bytes[which], which > 0 ? A.outgz[which].on_device() : g_bam.device, gz_carry[which],
                                       false, &u.out[which], &what))
          lib_fail(c, u, what, rc);
        else if (const int rc2 = fetch_wait(c, u.out[which], &gz_carry[which])) lib_fail(c, u, "fqg_*_output_wait", rc2);
      }
    if (!u.rc && u.r.code == FQG_E_WRONG_HEADER) u.wrong_header = locate_record(u.b[u.r.file].data, u.b[u.r.file].size, u.r.n_done).l[0];
    T[di].out += (timing ? now() : 0) - t3;
  }
  void work(size_t di, Unit& u) {
    fqg_ctx* c = ctx[di];
    const double t1 = timing ? now() : 0;
    fqg_frame* held[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    fqg_file_state states[6];
    for (int x = 0; x < 6; ++x) states[x] = A.pr[x].st;
    frame_unit(c, u, states, held);
    T[di].frame += (timing ? now() : 0) - t1;
    if (!u.rc && u.n > 0) transform_unit(di, c, u, states, held);
    else if (!u.rc) u.n = 0;
    for (int x = READ1; x <= INDEX3; ++x)
      if (cut[x]) {
        if (held[x]) fqg_frame_release(held[x]);
        cut[x]->release(u.b[x]);
      }
  }

  [[noreturn]] void run(size_t devices) {
    using UnitRun = OrderedRun<Unit>;
    // (fq_ordered.h: the units to whichever context is free, the results to this thread in unit order)
    UnitRun run(
        ctx.size(), window, [&](uint64_t seq, Unit& u, bool& last) { return next_unit(seq, u, last); },
        [&](size_t di, Unit& u) { work(di, u); },
        [&] {  // (a context may be waiting for an output buffer or for blocks, a cutter for a slot that stays held)
          out_pool.stop();
          for (int x = READ1; x <= INDEX3; ++x)
            if (cut[x]) cut[x]->abort();
        },
        [&](size_t di, const UnitRun::Waits& w) {
          if (timing) fprintf(fqhost::diag(), "fqgpu timing: context %zu: %llu units; waiting for blocks %.3f s, copy + framing %.3f s, transform %.3f s, output D2H %.3f s, handing over %.3f s\n",
                              di, (unsigned long long)w.items, w.fetch, T[di].frame, T[di].transform, T[di].out, w.hand_over);
        });
    InputEnd end[6];
    double t_main_wait = 0;
    const double t_loop = now();
    for (;;) {
      Unit u;
      const double tw = timing ? now() : 0;
      const bool more = run.next(u);
      if (timing) t_main_wait += now() - tw;
      if (!more) break;
      if (u.rc) {
        run.stop();
        if (u.long_line_file) refuse_long_line(A.file[u.long_line_file], u.long_line_record);
        FQ_PRINT_ERROR("GPU library failure in %s (%d)", u.err.c_str(), u.rc);
        fqhost::leave(kExitSys);
      }
      if (u.n > 0) {
        A.announce(u.r);
        for (int which = 0; which < 3; ++which)
          if (u.r.out_bytes[which] && !write_out(A.outgz, which, u.out[which]) && which > 0) {
            run.stop();
            FQ_PRINT_ERROR("%s.\n", A.outgz[which].error().c_str());  // GZ_WRITE's gzerror() text, src/fastq.c:211-235
            fqhost::leave(kExitSys);
          }
        A.count(u.r, [&] { run.stop(); }, [&] { return WrongHeader{(unsigned long)(4 * (u.seq * B + u.r.n_done + 1)), u.wrong_header}; });
      }
      for (OutText& o : u.out) out_pool.give(o.buf, o.cap);
      run.done();
      for (int x = READ1; x <= INDEX3; ++x) {  // (of the last unit taken: later ones, if any were handed out, are dropped)
        const Framed& f = u.f[x];
        end[x].drained = f.final && f.r.n_records == u.n;
        end[x].at_end = true;
        end[x].open_end = f.open_end;
        end[x].tail_lines = f.tail_lines;
        end[x].records = u.seq * B + f.r.n_records;
      }
      if (u.ends) break;
    }
    run.stop();
    if (timing) fprintf(fqhost::diag(), "fqgpu timing: the thread that writes: %.3f s in the loop, %.3f s of them waiting for the next unit\n", now() - t_loop, t_main_wait);
    A.finish(end, devices);
  }
};

}  // namespace

int main(int argc, char** argv) {
  fqhost::install_counted_output(argv);  // (fq_respawn.h: a run that starts over on input cut at the gzgets limits prints nothing twice)
  static int verbose = 0, paired = 0, help = 0, out_sam = 0, tenx = 0;
  fqg_barcode_params P;
  memset(&P, 0, sizeof(P));
  const char* file[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const char* outfile[3] = {nullptr, nullptr, nullptr};
  P.phred_encoding = 64;
  P.umi_read = P.cell_read = P.sample_read = -1;
  P.umi_offset = P.cell_offset = P.sample_offset = -1;
  P.read_offset[1] = P.read_offset[2] = -1;
  int num_input_files = 0;
  bool has_interleaved = false;
  opterr = 0;
  fprintf(stderr, "fastq_utils %s\n", "0.25.3");

  static struct option long_options[] = {{"verbose", no_argument, &verbose, 1},
                                         {"brief", no_argument, &verbose, 0},
                                         {"paired_end", no_argument, &paired, 1},
                                         {"single_end", no_argument, &paired, 0},
                                         {"sam", no_argument, &out_sam, 1},
                                         {"bam", no_argument, &out_sam, FQG_OUT_BAM},
                                         {"fastq", no_argument, &out_sam, 0},
                                         {"help", no_argument, &help, 1},
                                         {"umi_read", required_argument, 0, 'a'},
                                         {"umi_offset", required_argument, 0, 'b'},
                                         {"umi_size", required_argument, 0, 'c'},
                                         {"read1_offset", required_argument, 0, 'd'},
                                         {"read1_size", required_argument, 0, 'e'},
                                         {"read2_offset", required_argument, 0, 'f'},
                                         {"read2_size", required_argument, 0, 'g'},
                                         {"min_qual", required_argument, 0, 'h'},
                                         {"cell_read", required_argument, 0, 'i'},
                                         {"cell_offset", required_argument, 0, 'j'},
                                         {"cell_size", required_argument, 0, 'k'},
                                         {"read1", required_argument, 0, 'l'},
                                         {"read2", required_argument, 0, 'm'},
                                         {"index1", required_argument, 0, 't'},
                                         {"index2", required_argument, 0, 'v'},
                                         {"index3", required_argument, 0, 'u'},
                                         {"outfile1", required_argument, 0, 'n'},
                                         {"outfile2", required_argument, 0, 'o'},
                                         {"interleaved", required_argument, 0, 'z'},
                                         {"sample_read", required_argument, 0, 'p'},
                                         {"sample_offset", required_argument, 0, 'q'},
                                         {"sample_size", required_argument, 0, 'r'},
                                         {"phred_encoding", required_argument, 0, 's'},
                                         {"10x", no_argument, &tenx, 1},
                                         {0, 0, 0, 0}};
  auto set_input = [&](const char* name, int idx) {
    if (name && !file[idx]) num_input_files++;
    file[idx] = name;
  };
  for (;;) {
    int option_index = 0;
    const int c = getopt_long(argc, argv, "a:b:c:d:e:f:g:h:i:j:k:l:m:n:o:p:q:r:s:t:u:z:X", long_options, &option_index);
    if (c == -1) break;
    switch (c) {
      case 'X': tenx = 1; break;
      case 'z': {
        char tmps[1025];
        strncpy(tmps, optarg, 1024);
        tmps[1024] = 0;
        int xx = 0;
        char* token = strtok(tmps, ",");
        int refs[3] = {0, 0, 0};
        while (token != nullptr) {
          refs[xx] = read_index2read_idx(token);
          token = xx == 2 ? nullptr : strtok(nullptr, ",");
          ++xx;
        }
        if (xx != 2) {
          FQ_PRINT_ERROR("two file references should be passed to --interleaved");
          fqhost::leave(1);
        }
        P.interleaved[0] = refs[0];
        P.interleaved[1] = refs[1];
        has_interleaved = true;
        break;
      }
      case 'a': P.umi_read = read_index2read_idx(optarg); break;
      case 'b': P.umi_offset = atol(optarg); break;
      case 'c': P.umi_size = atol(optarg); break;
      case 'd': P.read_offset[READ1] = atol(optarg); break;
      case 'e': P.read_size[READ1] = atol(optarg); break;
      case 'f': P.read_offset[READ2] = atol(optarg); break;
      case 'g': P.read_size[READ2] = atol(optarg); break;
      case 'h': P.min_qual = atoi(optarg); break;
      case 'i': P.cell_read = read_index2read_idx(optarg); break;
      case 'j': P.cell_offset = atol(optarg); break;
      case 'k': P.cell_size = atol(optarg); break;
      case 'l': set_input(optarg, READ1); break;
      case 'm': set_input(optarg, READ2); break;
      case 't': set_input(optarg, INDEX1); break;
      case 'v': set_input(optarg, INDEX2); break;
      case 'u': set_input(optarg, INDEX3); break;
      case 'n': outfile[READ1] = optarg; break;
      case 'o': outfile[READ2] = optarg; break;
      case 'p': P.sample_read = read_index2read_idx(optarg); break;
      case 'q': P.sample_offset = atol(optarg); break;
      case 'r': P.sample_size = atol(optarg); break;
      case 's': P.phred_encoding = atoi(optarg); break;
      default: break;
    }
  }
  if (help) {
    print_usage();
    fqhost::leave(0);
  }
  FQ_PRINT_INFO("Validating options...");
  if (!file[READ1]) {  // validate_options, src/fastq_pre_barcodes.c:91-107
    FQ_PRINT_ERROR("missing input file (-read1)");
    fqhost::leave(1);
  }
  if (paired && !file[READ2]) {
    FQ_PRINT_ERROR("if paired_end is used then two fastq files should be provided - missing input file (-read2)");
    fqhost::leave(kExitParams);
  }
  if (!outfile[READ1]) {
    FQ_PRINT_ERROR("if single_end then -outfile1 should be provided");
    fqhost::leave(kExitParams);
  }
  FQ_PRINT_INFO("Options OK.");
  FQ_PRINT_INFO("input files %d", num_input_files);

  const char* dev = getenv("FQGPU_DEVICE");
  std::vector<int> devices = devices_from_env();  // FQGPU_DEVICES=0,1,..: record blocks over several GPUs
  if (has_interleaved) devices.clear();
  // One GPU, nothing said: the loop over record blocks all the same - every input has a reader of its own there (the serial
  // loop below reads them one after the other: 1.4 s against 0.9 - 1.0 s for 40 M reads and their index reads from tmpfs,
  // profiles/r07_multi_dev_legs.txt).  FQGPU_SERIAL_LOOP=1 keeps the serial loop, which is also what --interleaved input
  // runs through and a run that was started over on input cut at the gzgets limits (fq_respawn.h).
  const bool block_loop = !has_interleaved && !fqhost::reframing() && !getenv("FQGPU_SERIAL_LOOP");
  // (one context: a second one on the same GPU brought nothing that could be told from the noise - 200 M pairs to SAM 5.0 -
  // 6.1 s with one, 5.4 - 5.5 with two; 40 M reads 1.01 against 1.10 - and costs 30 ms to open; FQGPU_DEVICES=0,0 asks for it)
  if (devices.empty() && block_loop) devices.assign(1, dev ? atoi(dev) : 0);
  const bool multi = block_loop ? !devices.empty() : devices.size() > 1;
  int rc = fqg_open(multi ? devices[0] : (dev ? atoi(dev) : 0), &g_ctx);
  if (rc != 0) {
    FQ_PRINT_ERROR("no usable MI355X GPU (fqg_open: %d); this build has no CPU path", rc);
    fqhost::leave(kExitSys);
  }
  P.out_sam = out_sam;
  P.tenx = tenx;
  GzipMembers outgz[3];  // gzip level 4 like the reference's "w4", one member per 4 MiB block, all cores
  Batches A;
  A.file = file, A.P = &P, A.outgz = outgz, A.num_input_files = num_input_files, A.scale = has_interleaved ? 2 : 1;
  Source src[6];
  for (int x = READ1; x <= INDEX3; ++x)
    if (file[x]) {
      P.present[x] = 1;
      src[x].pr = &A.pr[x];
      if (!multi) src[x].in = new Input(g_ctx, file[x], piece_bytes(512));
    }
  if (has_interleaved && (!file[P.interleaved[0]] || !file[P.interleaved[1]])) {
    FQ_PRINT_ERROR("--interleaved refers to an input that was not given");
    fqhost::leave(kExitParams);
  }
  if (!out_sam) {
    for (int x = READ1; x <= READ2; ++x)
      if (outfile[x]) {
        if (!file[x]) {
          FQ_PRINT_ERROR("--outfile%d needs --read%d", x, x);
          fqhost::leave(kExitParams);
        }
        P.emit[x] = 1;
        // ("-": the reference's gzdopen(stdout, "wb") compresses at the default level; "w4" otherwise)
        if (!outgz[x].open(outfile[x], (outfile[x][0] == '-' && outfile[x][1] == 0) ? Z_DEFAULT_COMPRESSION : 4)) {
          FQ_PRINT_ERROR("Unable to open %s", outfile[x]);
          fqhost::leave(kExitParams);
        }
        // FQGPU_GZIP_GPU=1: the device compressor, in the loops that run on ONE context.  Over several contexts unit k
        // could cut its members only once the text lengths of units 0 .. k - 1 are known (docs/host_gzip.md section 3):
        // no device is handed over there and the host compressor runs
        if (devices.size() <= 1) outgz[x].device(FQ_GZIP_DEVICE(g_ctx));
      }
  } else if (out_sam == FQG_OUT_BAM) {
    // the header libbam makes of the two lines below (fqg_bam_header: one place for the @PG rule).  Device mode: several
    // contexts have no carry chain (above) and take the host compressor - and so must a run that such a run starts over
    std::string head(fqg_bam_header(argc, argv, nullptr, 0), '\0');
    fqg_bam_header(argc, argv, &head[0], head.size());
    const char* gz_gpu = getenv("FQGPU_GZIP_GPU");
    g_bam.on = true;
    g_bam.device = gz_gpu && atoi(gz_gpu) != 0 && devices.size() <= 1;
    if (!g_bam.device) setenv("FQGPU_GZIP_GPU", "0", 1);
    g_bam.host.open(stdout, Z_DEFAULT_COMPRESSION);
    if (g_bam.device) g_bam_header = head;
    else if (!g_bam.host.write(head.data(), head.size())) {
      FQ_PRINT_ERROR("unable to write the BAM file to stdout");
      fqhost::leave(kExitSys);
    }
  } else {
    printf("@HD\tVN:1.0 SO:unknown\n");
    printf("@PG\tID:1 PN:fastq_pre_barcodes CL:%s", argv[0]);
    for (int c = 1; c < argc - 1; c++) printf(" %s", argv[c]);  // (the reference drops the last word)
    printf("\n");
  }

  if (multi) BlockLoop(A, devices).run(std::set<int>(devices.begin(), devices.end()).size());

  // ---- the serial loop: --interleaved input, a run started over on re-framed input, FQGPU_SERIAL_LOOP=1 ----
  // (the text travels in pinned buffers that go round: per output one on its way from the GPU, two that wait for the
  // writer and the one it writes)
  OutPool out_pool(FQ_PINNED_ALLOC(g_ctx), 4 * outputs_per_batch(P));
  AsyncOut outq;
  outq.gz = outgz;
  outq.pool = &out_pool;
  outq.start();
  auto drain_or_die = [&] {
    if (!outq.drain()) {
      const char* why = "write error";
      for (int which = 1; which < 3; ++which)
        if (!outgz[which].error().empty()) why = outgz[which].error().c_str();
      FQ_PRINT_ERROR("%s.\n", why);  // GZ_WRITE's gzerror() text, src/fastq.c:211-235
      fqhost::leave(kExitSys);
    }
  };
  const bool timing = getenv("FQGPU_TIMING") != nullptr;
  double t_refill = 0, t_transform = 0, t_fetch = 0, t_hand = 0;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  auto step_of = [&](int x) { return (has_interleaved && (x == P.interleaved[0] || x == P.interleaved[1])) ? 2L : 1L; };
  for (int x = READ1; x <= INDEX3; ++x)
    if (file[x]) src[x].use = (has_interleaved && x == P.interleaved[1]) ? 1 : 0;

  std::vector<OutJob> in_flight;  // output of the last transform, on its way to the host
  std::string gz_carry[3] = {g_bam_header, std::string(), std::string()};  // device mode: the text the last batch left over, per output (the carry chain)
  g_bam.carry = &gz_carry[0];
  auto land_output = [&] {
    for (const OutJob& job : in_flight) {
      const double t_d = now();
      if (const int rc = fetch_wait(g_ctx, job.t, &gz_carry[job.which])) die_lib("fqg_*_output_wait", rc);
      const double t_e = now();
      outq.push(job);
      t_fetch += t_e - t_d;
      t_hand += now() - t_e;
    }
    in_flight.clear();
  };
  auto flush = [&] {
    land_output();
    drain_or_die();
  };
  g_before_respawn = flush;
  for (;;) {
    // every input needs a frame that holds the record its next iteration uses
    const double t_a = now();
    bool out_of_data = false;
    for (int x = READ1; x <= INDEX3 && !out_of_data; ++x)
      if (file[x]) {
        Source& s = src[x];
        while (!s.frame || s.use >= (long)s.avail) {
          if (!refill(s) && !s.frame) {
            out_of_data = true;
            break;
          }
          if (s.frame && s.use < (long)s.avail) break;
          if (s.exhausted && (!s.frame || s.use >= (long)s.avail)) {
            out_of_data = true;
            break;
          }
        }
      }
    if (out_of_data) break;
    uint64_t n = ~0ull;
    for (int x = READ1; x <= INDEX3; ++x)
      if (file[x]) {
        const Source& s = src[x];
        const uint64_t left = s.avail - (uint64_t)s.use;
        const long st = step_of(x);
        n = std::min<uint64_t>(n, (left + st - 1) / st);
      }
    if (n == 0 || n == ~0ull) break;
    const fqg_frame* frames[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    fqg_file_state states[6];
    uint64_t first[6] = {0, 0, 0, 0, 0, 0};
    memset(states, 0, sizeof(states));
    fqg_barcode_params Pb = P;
    for (int x = READ1; x <= INDEX3; ++x)
      if (file[x]) {
        frames[x] = src[x].frame;
        states[x] = A.pr[x].st;
        // the library adds +1 for the second interleaved reference itself
        first[x] = (uint64_t)src[x].use - ((has_interleaved && x == P.interleaved[1]) ? 1 : 0);
      }
    fqg_barcode_result r;
    land_output();  // (the transform writes the device buffers the previous batch's text is copied from)
    const double t_b = now();
    LIB(fqg_barcodes_transform(g_ctx, frames, states, first, &Pb, n, A.processed, &r));
    const double t_c = now();
    t_refill += t_b - t_a;
    t_transform += t_c - t_b;
    A.announce(r);
    // The text comes back on a stream of its own, beside the upload and framing of the NEXT pieces of input (the link
    // carries both directions at once: tools/kbench/duplex.hip); it is handed to the writer (stdout / gzip) when the
    // next batch is about to be transformed - land_output(), at the top of the loop - or the loop ends.  (Device mode:
    // the carry is the tail that landed with the previous batch: land_output() has run before this batch's transform.)
    for (int which = 0; which < 3; ++which)
      if (r.out_bytes[which]) {
        const double t_d = now();
        OutJob job;
        job.which = which;
        const char* what;
        if (const int rc = fetch_begin(g_ctx, out_pool, which, r.out_bytes[which], which > 0 ? outgz[which].on_device() : g_bam.device, gz_carry[which], true,
                                       &job.t, &what))
          die_lib(what, rc);
        in_flight.push_back(job);
        t_fetch += now() - t_d;
      }
    // (the header text of a wrong header: first line of that record in the file's current piece)
    A.count(r, flush, [&] {
      const Source& s = src[r.file];
      const uint64_t local = (uint64_t)s.use + r.n_done * step_of(r.file);
      return WrongHeader{(unsigned long)(4 * (s.records_before + local + 1)), locate_record(s.in->data(), s.in->size(), local).l[0]};
    });
    const bool ended_on_discard = has_interleaved && r.n_done < n;
    for (int x = READ1; x <= INDEX3; ++x)
      if (file[x]) {
        src[x].use += (long)r.n_done * step_of(x);
        if (ended_on_discard && x == P.interleaved[0]) src[x].use -= 1;  // no re-synchronising read after a discard
      }
  }
  flush();
  outq.stop();
  if (timing)
    fprintf(fqhost::diag(), "\nfqgpu timing: reading + framing %.3f s, transform %.3f s, output D2H %.3f s, waiting for the writer %.3f s; "
                    "the writer (gzip / stdout) worked %.3f s beside them\n", t_refill, t_transform, t_fetch, t_hand, outq.t_write);
  InputEnd end[6];
  for (int x = READ1; x <= INDEX3; ++x)
    if (file[x]) {
      const Source& s = src[x];
      end[x].drained = s.exhausted && (!s.frame || s.use >= (long)s.avail);
      end[x].at_end = !s.frame || s.use == (long)s.avail;
      end[x].one_beyond = has_interleaved && x == P.interleaved[1] && s.use == (long)s.avail + 1;
      end[x].open_end = s.f.open_end;
      end[x].tail_lines = s.f.tail_lines;
      end[x].records = s.records_before + s.avail;
    }
  A.finish(end, 1);
}
