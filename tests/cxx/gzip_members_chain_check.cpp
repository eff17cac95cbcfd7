// GzipMembers::write_members (host/fq_parallel.h) under the carry chain of fastq_pre_barcodes' device mode, without a
// device: a fake GzipDevice cuts the text at FQG_GZ_MEMBER_TEXT bytes and makes the members with zlib.
//
//   gzip_members_chain_check OUT.gz TAKEN.txt <taken> <unit bytes> ...
//
// A "context thread" compresses unit after unit (carry = the tail of the unit before; a unit without text makes no
// call, as in the program) and hands (members, tail) to the writer, which takes the first <taken> units (-1: all) and
// drops the rest - the context thread has compressed them all the same - then closes the file through the device.
// The file must inflate to the text of the units taken and be cut as ONE call on that text cuts it.  Exit status 0: both
// hold; OUT.gz and TAKEN.txt are left for the caller to look at.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fastq_utils_amd/host/fq_parallel.h"

struct fqg_ctx {
  std::string unit;               // the "store": what the producer call left
  std::vector<uint8_t> produced;  // members and tail of the last deflate call
  int calls = 0;
};

namespace {

constexpr size_t kMember = FQG_GZ_MEMBER_TEXT;

void zlib_member(const char* p, size_t n, std::vector<uint8_t>& out) {
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (deflateInit2(&zs, 1, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) abort();
  std::vector<uint8_t> buf(deflateBound(&zs, (uLong)n) + 32);
  static char none = 0;
  zs.next_in = reinterpret_cast<Bytef*>(const_cast<char*>(n ? p : &none));
  zs.avail_in = (uInt)n;
  zs.next_out = buf.data();
  zs.avail_out = (uInt)buf.size();
  if (deflate(&zs, Z_FINISH) != Z_STREAM_END) abort();
  out.insert(out.end(), buf.begin(), buf.begin() + (long)zs.total_out);
  deflateEnd(&zs);
}

// the contract of fqg_deflate (include/fqg.h)
int fake_run(fqg_ctx* c, const std::string& text, int final, fqg_deflate_result* out) {
  ++c->calls;
  c->produced.clear();
  const size_t n_full = text.size() / kMember, rest = text.size() % kMember;
  const size_t n_members = n_full + ((final && (rest || !n_full)) ? 1 : 0);
  for (size_t m = 0; m < n_members; ++m) zlib_member(text.data() + m * kMember, std::min(kMember, text.size() - m * kMember), c->produced);
  out->text_bytes = text.size();
  out->n_members = n_members;
  out->gz_bytes = c->produced.size();
  out->tail_bytes = final ? 0 : rest;
  c->produced.insert(c->produced.end(), text.end() - (long)out->tail_bytes, text.end());
  return 0;
}
int fake_deflate(fqg_ctx* c, const void* carry, uint64_t carry_bytes, const void* src, uint64_t nbytes, int, int final, fqg_deflate_result* out) {
  if (carry_bytes >= kMember) return FQG_ERR_ARG;
  std::string text(static_cast<const char*>(carry), carry_bytes);
  text.append(static_cast<const char*>(src), nbytes);
  return fake_run(c, text, final, out);
}
int fake_text_deflate(fqg_ctx* c, int, int, const void* carry, uint64_t carry_bytes, int final, fqg_deflate_result* out) {
  if (carry_bytes >= kMember) return FQG_ERR_ARG;
  return fake_run(c, std::string(static_cast<const char*>(carry), carry_bytes) + c->unit, final, out);
}
int fake_output(fqg_ctx* c, void* dst, uint64_t n) {
  if (n > c->produced.size()) return FQG_ERR_ARG;
  if (n) memcpy(dst, c->produced.data(), n);
  return 0;
}
const char* fake_error(const fqg_ctx*) { return "fake"; }

std::string unit_text(size_t k, size_t n) {  // FASTQ-like, different per unit
  std::string s;
  s.reserve(n + 64);
  for (size_t i = 0; s.size() < n; ++i) s += "@u" + std::to_string(k) + ":" + std::to_string(i) + "\nACGTTGCA" + std::string(i % 23, "ACGT"[i % 4]) + "\n+\nIIIIFFFF\n";
  s.resize(n);
  return s;
}

bool inflate_all(const std::vector<uint8_t>& gz, std::string& text, std::vector<size_t>& member_text) {
  size_t at = 0;
  while (at < gz.size()) {
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, 15 + 16) != Z_OK) return false;
    std::vector<uint8_t> buf(kMember + 64);
    zs.next_in = const_cast<Bytef*>(gz.data() + at);
    zs.avail_in = (uInt)(gz.size() - at);
    zs.next_out = buf.data();
    zs.avail_out = (uInt)buf.size();
    const int rc = inflate(&zs, Z_FINISH);
    const size_t used = zs.total_in, made = zs.total_out;
    inflateEnd(&zs);
    if (rc != Z_STREAM_END) return false;
    text.append(reinterpret_cast<const char*>(buf.data()), made);
    member_text.push_back(made);
    at += used;
  }
  return true;
}

std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  uint8_t buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const long taken = atol(argv[3]);
  std::vector<size_t> sizes;
  for (int i = 4; i < argc; ++i) sizes.push_back(strtoull(argv[i], nullptr, 10));
  setenv("FQGPU_GZIP_GPU", "1", 1);
  fqg_ctx ctx;
  fqhost::GzipMembers out;
  if (!out.open(argv[1], 4)) return 3;
  out.device(fqhost::GzipDevice{&ctx, fake_deflate, fake_text_deflate, fake_output, fake_error});
  if (!out.on_device()) return 4;

  // the context thread: every unit, in order, the carries its own
  struct Unit {
    bool has_text = false;
    std::vector<uint8_t> buf;  // members, then the tail
    size_t gz = 0, tail = 0;
  };
  std::vector<Unit> units(sizes.size());
  std::string carry, taken_text;
  for (size_t k = 0; k < sizes.size(); ++k) {
    ctx.unit = unit_text(k, sizes[k]);
    if (taken < 0 || (long)k < taken) taken_text += ctx.unit;
    if (ctx.unit.empty()) continue;
    fqg_deflate_result r;
    if (fake_text_deflate(&ctx, FQG_TEXT_RECORDS, 1, carry.data(), carry.size(), 0, &r) != 0) return 5;
    Unit& u = units[k];
    u.has_text = true;
    u.gz = r.gz_bytes;
    u.tail = r.tail_bytes;
    u.buf.resize(u.gz + u.tail);
    if (fake_output(&ctx, u.buf.data(), u.buf.size()) != 0) return 5;
    carry.assign(reinterpret_cast<const char*>(u.buf.data()) + u.gz, u.tail);
  }
  // the writer: the units it takes; the tail of the last of them is what close() compresses
  const int calls_before = ctx.calls;
  for (size_t k = 0; k < units.size() && (taken < 0 || (long)k < taken); ++k) {
    const Unit& u = units[k];
    if (!u.has_text) continue;
    const char* p = reinterpret_cast<const char*>(u.buf.data());
    if (!out.write_members(p, u.gz, p + u.gz, u.tail)) return 6;
  }
  if (ctx.calls != calls_before) return 7;  // (the writer calls into no context before close())
  if (!out.close()) return 8;
  if (ctx.calls > calls_before + 1) return 7;

  FILE* t = fopen(argv[2], "wb");
  if (!t || fwrite(taken_text.data(), 1, taken_text.size(), t) != taken_text.size() || fclose(t) != 0) return 3;
  const std::vector<uint8_t> file = slurp(argv[1]);
  std::string text;
  std::vector<size_t> cut;
  if (!inflate_all(file, text, cut)) return 10;
  if (text != taken_text) return 11;
  fqg_ctx whole;
  fqg_deflate_result r;
  if (fake_deflate(&whole, nullptr, 0, taken_text.data(), taken_text.size(), FQG_MEM_HOST, 1, &r) != 0) return 5;
  if (cut.size() != r.n_members || file != whole.produced) return 12;
  for (size_t m = 0; m + 1 < cut.size(); ++m)
    if (cut[m] != kMember) return 13;
  if (cut.empty() || cut.back() > kMember || (cut.size() > 1 && cut.back() == 0)) return 13;
  printf("%zu units, %ld taken, %zu bytes of text, %zu members\n", sizes.size(), taken, taken_text.size(), cut.size());
  return 0;
}
