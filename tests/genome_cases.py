"""Organism-file cases shared by test_genome_core_host.py (mg_genome_core.h compiled for the host) and test_gpu_genome_ingest.py
(the kernels).  A case is a list of files as bytes; what is expected of a file is always build_db.genome_bases of that file written
to disk — or, for a file that holds a byte on which Python's text mode and the device's byte rules part, and for a file on which
genome_bases RAISES (a header line without a name: formats.read_sequences takes line[1:].split()[0]), that it is flagged undecided
(and that the files next to it still parse)."""
import os

import numpy as np

from metalign_amd import build_db


def seq(n, seed=0, alphabet=b"ACGT"):
    rng = np.random.default_rng(1000 + seed)
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n).astype(np.uint8))


def fasta(records, width=60, newline=b"\n", final_newline=True):
    out = []
    for i, r in enumerate(records):
        out.append(b">rec%d some description" % i)
        out.extend(r[j:j + width] for j in range(0, len(r), width))
    text = newline.join(out)
    return text + (newline if final_newline and out else b"")


OK = b">ok\nACGTACGT\nTTGGCCAA\n"


def n_lines(n, final_newline=True):
    """A file of exactly n lines: a header and n - 1 short sequence lines."""
    lines = [b">x"] + [seq(4 + (i % 5), i) for i in range(n - 1)]
    return b"\n".join(lines) + (b"\n" if final_newline else b"")


def _alignments():
    # 17-byte lines ('\n' included): every line starts one residue further modulo 16; leading blanks move the stripped start too
    lines = [b">h"] + [b" " * (i % 3) + seq(16 - (i % 3), i) for i in range(40)]
    return b"\n".join(lines) + b"\n"


CASES = {
    "empty_file": [b""],
    "gt_alone": [b">"],
    "gt_alone_newline": [OK, b">\n", OK],  # (genome_bases raises on a header without a name: left to the host, like the undecided)
    "nameless_headers": [b">a\nAC\n> \t\nGT\n", b">a\nAC\n>\r\n", b">a\nAC\n>  ", b">a\nAC\n>", b"> x\nAC\n"],
    "header_last_line": [b">a\nACGT\n>b", b">a\nACGT\n>b\n"],
    "no_header": [b"ACGT\nGGCC\n"],
    "junk_before_header": [b"junk\n  more junk \n\n>a\nAC\nGT\n"],
    "two_records": [b">a\nACGT\nAC\n>b\nGG\n"],
    "three_records": [b">a\nACGT\n>b\nGG\nTT\n>c\nA\n"],
    "many_records_some_empty": [b">a\n>b\nAC\n>c\n>d\n>e\nGT\n>f\n", fasta([seq(100 + 7 * i, i) if i % 3 else b"" for i in range(40)])],
    "only_empty_records": [b">a\n>b\n>c\n"],
    "blank_lines_inside": [b">a\nAC\n\n   \nGT\n\t\n>b\n\n \t \nTT\n\n"],
    "spaces_and_tabs": [b">a\n  AC GT\t\n\tA  C\t \n \x0b\x0cTT\x0c\x0b \n"],
    "crlf": [fasta([seq(130, 1), b"", seq(61, 2)], newline=b"\r\n"), b">a\r\nAC\r\n\r\nGT"],
    "no_final_newline_then_file": [b">a\nACGT", b">b\nGGCC\n", b"TTTT", b">c\nAA", b">", b">d\nCC"],
    "lower_case_and_iupac": [b">a\nacgtnNRYKMswbdhv\nACGTU*-.\n>b\nnnnn\n"],
    "line_lengths": [b">a\n" + b"\n".join(seq(n, n) for n in (63, 64, 65, 129, 1, 7, 8, 9, 15, 16, 17, 128)) + b"\n",
                     b">a\n " + seq(63, 3) + b" \n  " + seq(64, 4) + b"\n\t" + seq(65, 5) + b"\t\t\n" + seq(129, 6)],
    "line_starts_mod_16": [_alignments(), b"j\n" + _alignments(), b"jjjjjjj\n" + _alignments()],
    "lines_255_256_257": [n_lines(255), n_lines(256), n_lines(257), n_lines(255, False), n_lines(256, False), n_lines(257, False)],
    "boundary_on_256th_line": [n_lines(255), OK, n_lines(255, False), OK, n_lines(256), OK],
    "files_1": [fasta([seq(500, 11), seq(300, 12)], width=70)],
    "files_2": [fasta([seq(500, 13)], width=80), fasta([seq(10, 14), seq(1000, 15)], width=61, final_newline=False)],
    "files_300": [(b"" if i % 17 == 5 else fasta([seq(20 + i % 50, i + j) for j in range(i % 4)], width=30, final_newline=i % 3 != 0))
                  for i in range(300)],
    "empty_file_between": [b">a\nAC\n", b"", b">b\nGT\n"],
    "undecided_lone_cr": [OK, b">a\nAC\rGT\n", OK],
    "undecided_cr_ends_file": [b">a\nACGT\r", b"\n>b\nAA\n", OK],
    "undecided_0x1d": [OK, b">a\nAC\x1dGT\n", OK],
    "undecided_0xe9_in_header": [OK, b">caf\xe9\nACGT\n", OK],
}


def undecided(data):
    """The three kinds of bytes a file is not decided on the device for."""
    return any(b >= 0x80 or 0x1c <= b <= 0x1f or (b == 0x0d and data[i + 1:i + 2] != b"\n") for i, b in enumerate(data))


def expected(files, tmp_dir):
    """Per file: bytes(build_db.genome_bases(the file on disk)), or None for a file the device must leave undecided."""
    out = []
    for i, data in enumerate(files):
        if undecided(data):
            out.append(None)
            continue
        p = os.path.join(str(tmp_dir), "f%d.fna" % i)
        with open(p, "wb") as fh:
            fh.write(data)
        try:
            out.append(bytes(np.asarray(build_db.genome_bases(p), dtype=np.uint8)))
        except IndexError:  # a header line without a name: the definition raises, nothing is defined
            out.append(None)
    return out


def self_check():
    """The case list covers what it claims to (cheap; both tests call it)."""
    assert [undecided(f) for f in CASES["undecided_cr_ends_file"]] == [True, False, False]
    assert sum(undecided(f) for c in CASES.values() for f in c) == 4
    assert {len(ln.strip()) for f in CASES["line_lengths"] for ln in f.split(b"\n")} >= {63, 64, 65, 129}
    starts = set()
    for f in CASES["line_starts_mod_16"]:
        at = 0
        for ln in f.split(b"\n"):
            starts.add(at % 16)
            at += len(ln) + 1
    assert starts == set(range(16))
    assert [f.count(b"\n") + (not f.endswith(b"\n")) for f in CASES["lines_255_256_257"]] == [255, 256, 257] * 2
    assert len(CASES["files_300"]) == 300 and b"" in CASES["files_300"]
