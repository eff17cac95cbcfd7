// TEST DRIVER: pinned memory that runs out under the two cutters (fastq_utils_amd/host/fq_multi.h, fq_blocks.h: one
// PinnedQueue, fq_input.h) - without a GPU: the pinned allocation is malloc, which returns nothing from its K-th call
// on.  Also under the sanitizers (tests/test_sanitizers.py).
// argv: file pieces|blocks size K   (size: bytes of a piece / records of a block)
// Three consumers over eight slots, each holding the item it works on while it asks for the next one - with fewer
// slots than consumers nobody would ever release one.  The run must end by itself: the queue fails, the consumer that
// learns of it says "unable to allocate pinned memory" and leaves with status 2 (fqhost::leave).  A run that comes to
// the end of the file instead prints "no failure" and returns 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>

#include "../../fastq_utils_amd/host/fq_blocks.h"
#include "../../fastq_utils_amd/host/fq_multi.h"

static std::atomic<long> g_calls{0};
static long g_fail_from = 0;

extern "C" void* fqg_host_alloc(fqg_ctx*, size_t bytes) { return ++g_calls >= g_fail_from ? nullptr : malloc(bytes ? bytes : 1); }
extern "C" void fqg_host_free(fqg_ctx*, void* p) { free(p); }

template <class Source, class Item>
static void consume(Source& src) {
  std::atomic<unsigned long long> seen{0};
  auto work = [&] {
    Item held, it;
    bool have = false;
    while (src.next(&it)) {
      if (have) src.release(held);
      for (size_t i = 0; i < it.size; ++i) seen += it.data[i] == '\n';
      held = it;
      have = true;
      if (it.final) break;
    }
    if (have) src.release(held);
  };
  std::thread a(work), b(work), c(work);
  a.join();
  b.join();
  c.join();
  printf("no failure (%llu lines)\n", seen.load());
}

int main(int argc, char** argv) {
  if (argc < 5) return 9;
  const uint64_t size = strtoull(argv[3], nullptr, 10);
  g_fail_from = atol(argv[4]);
  if (!strcmp(argv[2], "pieces")) {
    fqhost::AlignedPieces src(nullptr, argv[1], (size_t)size, 8);
    consume<fqhost::AlignedPieces, fqhost::Piece>(src);
  } else {
    fqhost::RecordBlocks src(nullptr, argv[1], 8);
    src.start(size);
    consume<fqhost::RecordBlocks, fqhost::Block>(src);
  }
  return 0;
}
