"""CPU-only checks of the boundary: libfqgpu.so loads without a GPU, exports every function that
include/fqg.h declares, and refuses to open a context when there is no device (no CPU path)."""
import ctypes
import os
import re

import pytest

import fastq_utils_amd as fq
from tests.util import REPO


def declared_functions():
    text = open(os.path.join(REPO, "include", "fqg.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fqg_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert declared_functions() == sorted(fq.abi.EXPORTS)


def test_library_exports_every_declared_symbol():
    lib = fq.abi.load()
    for name in declared_functions():
        assert hasattr(lib, name), name
    assert lib.fqg_abi_version() == 1


def test_struct_layouts_match_the_header():
    assert ctypes.sizeof(fq.abi.Record) == 32
    assert ctypes.sizeof(fq.abi.ValidateResult) == 64
    assert ctypes.sizeof(fq.abi.FileState) == 16
    assert ctypes.sizeof(fq.abi.IndexResult) == 32


def test_probes_follow_the_reference_ladder():
    L = fq.abi.load()
    assert L.fqg_probe_readname_format(b"A80910ABXX:2:1:20677:2129 1:N:0:ACGT\n") == fq.abi.NAME_CASAVA18
    assert L.fqg_probe_readname_format(b"12345\n") == fq.abi.NAME_INTEGER
    assert L.fqg_probe_readname_format(b"read_without_suffix\n") == fq.abi.NAME_INTEGER  # NOP == 2
    assert L.fqg_probe_readname_format(b"read/1\n") == fq.abi.NAME_DEFAULT
    assert L.fqg_probe_space(b"T0123012301\n") == fq.abi.SPACE_COLOUR
    assert L.fqg_probe_space(b"ACGTACGT\n") == fq.abi.SPACE_SEQ
    st = fq.abi.probe_first_record(b"@r/1\nACGT\n+\nIIII\n", True)
    assert (st.readname_format, st.space, st.is_pe) == (fq.abi.NAME_DEFAULT, fq.abi.SPACE_SEQ, 1)


def test_no_gpu_means_no_context():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(fq.abi.FqgError):
        fq.Context(0)


COMPAT_EXPORTS = [
    "fastq_print_version", "fastq_new_entry", "fastq_write_entry", "get_elength", "fastq_index_delete",
    "fastq_index_lookup_header", "fastq_get_readname", "fastq_read_entry", "fastq_new_entry_stats",
    "fastq_validate_entry", "fastq_read_next_entry", "fastq_new", "fastq_destroy", "fastq_is_pe",
    "fastq_index_readnames", "fastq_write_entry2stdout", "fastq_qualRange2enc", "fastq_open", "GZ_WRITE",
    "index_mem", "encodings", "new_hashtable", "get_next_object", "delete", "get_object", "insere",
    "free_hashtable", "reset_hashtable", "init_hash_traversal", "next_hash_object", "next_hashnode",
    "hashtable_stats",
    # src/fastq.h:151-155
    "fastq_seek_copy_read", "fastq_rewind", "fastq_quick_copy_entry",
    # src/range_list.h:150-162 (intersect_rl is declared there but defined nowhere in the reference)
    "new_rl", "copy_rl", "free_rl", "rl_all", "display_tree", "set_in_rl", "in_rl", "freeze_rl", "minus_rl",
    "rl_next_in_bigger",
]


def test_compat_library_exports_the_reference_api():
    """libfastq_gpu.so carries the names of src/fastq.h:84-158 and src/hash.h:64-78 (no compute call here)."""
    import ctypes
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fastq_utils_amd", "libfastq_gpu.so")
    assert os.path.exists(path), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(path)
    for name in COMPAT_EXPORTS:
        assert hasattr(lib, name), name


def test_compat_header_layouts_match_the_reference_headers(tmp_path):
    """Same struct layouts as the reference's own headers: a tiny program prints sizeof / offsetof under our header,
    and must print what the same program printed under the reference's fastq.h + range_list.h
    (tests/golden/compat_header_layouts.txt, recorded with gcc on x86-64 Linux)."""
    import os
    import subprocess

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    body = r'''
#include <stdio.h>
#include <stddef.h>
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(FASTQ_ENTRY), offsetof(FASTQ_ENTRY, hdr2), offsetof(FASTQ_ENTRY, seq),
         offsetof(FASTQ_ENTRY, qual), offsetof(FASTQ_ENTRY, read_len), offsetof(FASTQ_ENTRY, offset));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(FASTQ_FILE), offsetof(FASTQ_FILE, cline),
         offsetof(FASTQ_FILE, filename), offsetof(FASTQ_FILE, max_rl), offsetof(FASTQ_FILE, min_qual),
         offsetof(FASTQ_FILE, num_rds), offsetof(FASTQ_FILE, rdlen_ctr), offsetof(FASTQ_FILE, is_pe),
         offsetof(FASTQ_FILE, space));
  printf("%zu %zu %zu %zu %zu\n", sizeof(struct hashtable_s), offsetof(struct hashtable_s, size),
         offsetof(struct hashtable_s, n_entries), sizeof(hashnode), sizeof(INDEX_ENTRY));
  printf("%zu %zu %zu %zu %zu %d %d\n", sizeof(RL_Tree), offsetof(RL_Tree, size), offsetof(RL_Tree, mem_alloc),
         offsetof(RL_Tree, root_i), sizeof(RL_Node), (int)IN, (int)OUT);
  return 0;
}
'''
    src = tmp_path / "ours.c"
    src.write_text('#include "fastq_gpu_compat.h"' + body)
    exe = tmp_path / "ours"
    subprocess.run(["gcc", "-w", "-I", os.path.join(repo, "include"), "-o", str(exe), str(src)], check=True)
    ours = subprocess.run([str(exe)], capture_output=True, check=True).stdout
    with open(os.path.join(repo, "tests", "golden", "compat_header_layouts.txt"), "rb") as f:
        assert ours == f.read()


def test_reference_unit_test_program_runs_on_the_compat_library():
    """src/fastq_tests.c - the reference's only C test (hash.h + range_list.h, run_tests.sh:512) - compiled from the
    reference's source against the reference's headers and linked with libfastq_gpu.so (oracle/Makefile): same
    stdout, stderr and exit status as the same program linked with the reference's own objects.  Needs no GPU."""
    import subprocess

    a = os.path.join(REPO, "oracle", "_ref", "fastq_tests")
    b = os.path.join(REPO, "oracle", "_ref", "fastq_tests_on_libfastq_gpu")
    if not (os.path.exists(a) and os.path.exists(b)):
        pytest.skip("oracle/_ref/fastq_tests* not built (needs the reference checkout at build time)")
    ra = subprocess.run([a], capture_output=True, timeout=60)
    rb = subprocess.run([b], capture_output=True, timeout=60)
    assert (ra.returncode, ra.stdout, ra.stderr) == (rb.returncode, rb.stdout, rb.stderr)
    assert b"Size:3 -[1,100]" in ra.stdout
