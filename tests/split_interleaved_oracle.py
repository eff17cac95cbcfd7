"""fastq_split_interleaved (reference src/fastq_split_interleaved.c) stated in Python, for the tests.  The record loop
is fastq_info's interleaved loop (src/fastq_info.c:72-101) plus two writes, so findings and stderr come from the
restated fastq_info in oracle/liboracle_fq.so ("file pe" with -e -q: nothing fails behind the loop); the two output
texts are a plain de-interleave of the lines as C strings."""
import os

from oracle import loader as orc
from tests import split_gen
from tests.util import read_image

VERSION = "fastq_utils 0.25.3\n"
USAGE = "\nERROR: Usage: fastq_split_interleaved interleaved_fastq out_prefix\n"
SUMMARY_RULE = "------------------------------------\n"


def run(args, cwd, image=None):
    """dict(exit, stdout, stderr, files: name -> bytes, or None where the content is not defined).  `image`: the inflated
    input, when the caller has it already."""
    if len(args) != 2:
        return {"exit": 1, "stdout": "", "stderr": VERSION + USAGE, "files": {}}
    path, prefix = args
    err = VERSION + "Paired-end interleaved\n"
    if image is None:
        if not os.path.isfile(os.path.join(cwd, path)):
            return {"exit": 1, "stdout": "", "stderr": err + "\nERROR: Unable to open %s\n" % path, "files": {}}
        image = read_image(os.path.join(cwd, path))
    names = [prefix + "_1.fastq.gz", prefix + "_2.fastq.gz"]
    if not os.path.isdir(os.path.join(cwd, os.path.dirname(prefix))):
        return {"exit": 1, "stdout": "", "stderr": err + "\nERROR: Unable to open %s\n" % names[0], "files": {}}
    r = orc.fastq_info(image, path, None, "pe", orc.ARG2_PE, orc.FLAG_E | orc.FLAG_Q)
    assert r["stderr"].startswith(err)
    if r["exit"] != 0:
        return {"exit": r["exit"], "stdout": "", "stderr": r["stderr"], "files": {n: None for n in names}}
    # (a NUL byte at a record start ends the file there, src/fastq.c:250)
    lines, kept = split_gen.lines_of(image), []
    for k in range(0, len(lines) - len(lines) % 4, 4):
        if lines[k][:1] == b"\0":
            break
        kept += lines[k:k + 4]
    a, b = split_gen.deinterleave(b"".join(kept))
    return {"exit": 0, "stdout": "\n", "stderr": r["stderr"].split(SUMMARY_RULE)[0], "files": {names[0]: a, names[1]: b}}
