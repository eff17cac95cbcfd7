// TEST DRIVER: FastqSource (fastq_utils_amd/host/fq_source.h), the one place where the host programs open an input
// and read inflated bytes from it; no GPU and nothing of the library, also under the sanitizers
// (tests/test_sanitizers.py).
// argv: path reference want count_lines bgzf limit   ("-" as path: stdin; "-" as limit: none)
// Reads the input in calls of `want` bytes (a bgzip'd input read block by block is asked for at least 128 KiB, as
// fq_input.h does: it delivers whole blocks) and checks, against zlib's gzread of `reference` cut at the limit:
// the bytes are the same; at_end comes with the call that delivers the last byte, neither earlier nor later; with
// count_lines, the runs of every call tile its bytes and every run's count is what a recount of its bytes gives.
// Prints "<calls> <bytes> ok" or the first violation (exit 1); a failed source: its message on stderr, exit 2.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../fastq_utils_amd/host/fq_source.h"

int main(int argc, char** argv) {
  if (argc < 7) return 9;
  size_t want = strtoull(argv[3], nullptr, 10);
  const bool count = atoi(argv[4]) != 0;
  fqhost::FastqSource::Options opt;
  opt.bgzf = atoi(argv[5]) != 0;
  if (strcmp(argv[6], "-") != 0) opt.limit = strtoull(argv[6], nullptr, 10);
  std::string whole;
  {
    gzFile g = gzopen(argv[2], "r");
    if (!g) return 8;
    char buf[1 << 16];
    int got;
    while ((got = gzread(g, buf, sizeof buf)) > 0) whole.append(buf, (size_t)got);
    gzclose(g);
  }
  if (whole.size() > opt.limit) whole.resize((size_t)opt.limit);

  fqhost::FastqSource src(argv[1], opt);
  if (src.kind() == fqhost::FastqSource::kBgzf) want = std::max<size_t>(want, 1u << 17);
  const std::unique_ptr<char[]> mem(new char[want ? want : 1]);
  char* const buf = mem.get();
  size_t total = 0;
  unsigned long long calls = 0;
  bool at_end = false;
  while (!at_end) {
    fqhost::FastqSource::Lines runs;
    const size_t n = src.read(buf, want, &at_end, count ? &runs : nullptr);
    ++calls;
    if (src.failed()) {
      fprintf(stderr, "%s\n", src.error().c_str());
      return 2;
    }
    if (n > want) return printf("call %llu: %zu bytes where %zu were asked for\n", calls, n, want), 1;
    if (total + n > whole.size() || whole.compare(total, n, buf, n) != 0) return printf("call %llu: bytes differ from the file at %zu\n", calls, total), 1;
    total += n;
    if (at_end != (total == whole.size())) return printf("call %llu: at_end %d with %zu of %zu bytes delivered\n", calls, (int)at_end, total, whole.size()), 1;
    size_t at = 0;
    for (const fqhost::FastqSource::LineRun& r : runs) {
      if (r.begin != at || r.end <= r.begin || r.end > n) return printf("call %llu: run [%zu, %zu) behind %zu of %zu bytes\n", calls, r.begin, r.end, at, n), 1;
      if (r.lines != fqhost::FastqSource::count_lines(buf + r.begin, buf + r.end))
        return printf("call %llu: run [%zu, %zu) reports %llu lines\n", calls, r.begin, r.end, (unsigned long long)r.lines), 1;
      at = r.end;
    }
    if (count && at != n) return printf("call %llu: runs cover %zu of %zu bytes\n", calls, at, n), 1;
  }
  printf("%llu %zu ok\n", calls, total);
  return 0;
}
