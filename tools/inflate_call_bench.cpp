// inflate_call_bench - one BGZF file inflated both ways in one process (tools/inflate_gpu_quick.py builds and runs it):
//   device   fqg_bgzf_inflate + fqg_inflate_output into a std::vector, wall time; k_inflate_blocks from fqg_profile_read
//   host     fqhost::bgzf_inflate_parallel (zlib on the host's threads), wall time
// RUNS + 1 rounds of each, the first not counted; the two streams must be the same bytes.  One JSON object on stdout.
//   inflate_call_bench FILE RUNS
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../fastq_utils_amd/host/bam_input.h"

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int runs = atoi(argv[2]);
  FILE* f = fopen(argv[1], "rb");
  std::vector<uint8_t> raw;
  if (!f || !fqbam::read_all(f, raw)) return 2;
  fqg_ctx* ctx = nullptr;
  if (fqg_open(0, &ctx) != 0) return 3;
  std::vector<uint8_t> dev, host;
  std::string kern, call, upto, hostms;
  fqg_inflate_result r;
  memset(&r, 0, sizeof(r));
  for (int rep = 0; rep <= runs; ++rep) {
    fqg_profile_enable(ctx, 1);
    fqg_profile_reset(ctx);
    const double t0 = now_ms();
    if (fqg_bgzf_inflate(ctx, raw.data(), raw.size(), &r) != 0 || r.bad_block != UINT64_MAX) return 4;
    const double t1 = now_ms();
    dev.resize(r.out_bytes);
    if (fqg_inflate_output(ctx, 0, dev.data(), r.out_bytes) != 0) return 4;
    const double t2 = now_ms();
    fqg_kernel_time kt[64];
    size_t n = 0;
    fqg_profile_read(ctx, kt, 64, &n);
    fqg_profile_enable(ctx, 0);
    double k_ms = 0;
    for (size_t i = 0; i < n && i < 64; ++i)
      if (!strcmp(kt[i].name, "k_inflate_blocks")) k_ms = kt[i].total_ms;
    const double h0 = now_ms();
    if (!fqhost::bgzf_inflate_parallel(raw, host)) return 5;
    const double h1 = now_ms();
    if (!rep) continue;
    char buf[64];
    snprintf(buf, sizeof(buf), "%s%.3f", kern.empty() ? "" : ", ", k_ms), kern += buf;
    snprintf(buf, sizeof(buf), "%s%.3f", upto.empty() ? "" : ", ", t1 - t0), upto += buf;
    snprintf(buf, sizeof(buf), "%s%.3f", call.empty() ? "" : ", ", t2 - t0), call += buf;
    snprintf(buf, sizeof(buf), "%s%.3f", hostms.empty() ? "" : ", ", h1 - h0), hostms += buf;
  }
  if (dev != host) return 6;
  printf("{\"raw_bytes\": %llu, \"blocks\": %llu, \"out_bytes\": %llu, \"k_inflate_blocks_ms\": [%s], \"fqg_bgzf_inflate_ms\": [%s], "
         "\"device_call_ms\": [%s], \"host_inflate_ms\": [%s]}\n",
         (unsigned long long)r.raw_bytes, (unsigned long long)r.n_blocks, (unsigned long long)r.out_bytes, kern.c_str(), upto.c_str(),
         call.c_str(), hostms.c_str());
  fqg_close(ctx);
  fqbam::leave(0);
}
